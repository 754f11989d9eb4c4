"""The training objective on the MI355X (tcs_loss.hip through tcs_mi355.losses): the quarter-resolution targets bit-equal to the
torch CPU ops, each loss and training_objective against the reference's numbers (tests/golden/losses.npz) and the fp64 restatement
of test_losses_host.py, bit-equal repeated calls, the stacked fast path against separate tensors, the non-finite flag, and an
end-to-end frame of TCStereo.forward(test_mode=False)."""
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_losses_host import (assert_matches, case_inputs, golden, grad_xy, median_pool4, normal_xy, quarter_valid, restate,
                              targets)

pytestmark = pytest.mark.gpu

SEQ_KEYS = ("epe", "epe_refine", "epe_init", "1px", "3px", "5px", "1px_refine", "3px_refine", "5px_refine")
INIT_KEYS = ("init_loss", "init_gt_loss", "init_nm_loss", "forward_mask_rate")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from tcs_mi355 import native
    native.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    return golden()


def _on(case, dev, iters):
    """A make_loss_case on the device, laid out as forward(test_mode=False) returns it (list entries are views of stacks)."""
    t = {k: torch.from_numpy(v).to(dev) for k, v in case.items()}
    out = {"flow_predictions": [[t["up"][i, 0], t["up"][i, 1]] for i in range(iters)],
           "flow_q_predictions": [[t["q"][i, 0], t["q"][i, 1]] for i in range(iters)],
           "disp_grad_q_predictions": [t["grad"][i] for i in range(iters)],
           "flow_mono": t["flow_mono"], "flow_init": t["flow_init"], "cost_volume": t["cost_volume"]}
    return t, out


def _cases(gold):
    return [(i, [int(v) for v in c]) for i, c in enumerate(gold["cases"])]


def test_targets_bit_equal_to_torch(dev, gold):
    from tcs_mi355 import ops
    for i, c in _cases(gold):
        case = case_inputs(c)
        flow, valid = torch.from_numpy(case["flow"]), torch.from_numpy(case["valid"])
        v, g, gm, n, nm = targets(flow, valid)
        got = [x.cpu() for x in ops.loss_targets(flow.to(dev), valid.to(dev), ops.VALID_TRAINER)]
        want = (g, None, gm, None, quarter_valid(v, True), quarter_valid(v, False))
        for j, (a, b) in enumerate(zip(got, want)):
            if b is not None:
                assert a.shape == b.shape and torch.equal(a, b), (i, j)
        # the normal: bit-equal to the fused 2-norm written out (what PyTorch's vectorised CPU norm computes; its scalar tail and
        # other vector widths round differently), within an ulp of F.normalize on this CPU; the mask rule bit-exact on it
        fused = median_pool4(normal_fused(-flow))
        assert torch.equal(got[1], fused), i
        assert torch.allclose(got[1], n, rtol=3e-7, atol=1e-7), i
        assert torch.equal(got[3], (fused[:, :1] / fused[:, 2:] < 5) & (fused[:, 1:2] / fused[:, 2:] < 5)), i
        assert torch.equal(got[3], nm), i
        # the full-resolution entry on the trainer's own maps (gt_targets), C = 2 and 3, bool and float valid masks
        for gt in (grad_xy(-flow), normal_xy(-flow)):
            for vv, mode in ((v, ops.VALID_BOOL), (v.float(), ops.VALID_VALUES)):
                pooled, gmask, vd, vs = ops.loss_targets_full(gt.to(dev), vv.to(dev), mode)
                p = median_pool4(gt)
                assert torch.equal(pooled.cpu(), p), i
                if gt.shape[1] == 2:
                    assert torch.equal(gmask.cpu(), (p[:, :1] < 5) & (p[:, 1:] < 5))
                else:
                    assert torch.equal(gmask.cpu(), (p[:, :1] / p[:, 2:] < 5) & (p[:, 1:2] / p[:, 2:] < 5))
                assert torch.equal(vd.cpu(), F.max_pool2d(v.float(), 4, 4, 0).bool())
                assert torch.equal(vs.cpu(), F.interpolate(v.float(), scale_factor=0.25, mode="bilinear", align_corners=True) == 1)


def test_median_pool_bit_equal_with_ties_and_nan(dev):
    from tcs_mi355 import ops
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-3, 4, (2, 3, 24, 36), generator=g).float() * 0.5          # many ties
    x[0, 0, 1, 1] = float("nan")
    x[1, 2, 5, 9] = float("inf")
    valid = torch.ones(2, 1, 24, 36, dtype=torch.bool)
    pooled, *_ = ops.loss_targets_full(x.to(dev), valid.to(dev), ops.VALID_BOOL)
    assert torch.equal(pooled.cpu().nan_to_num(7.0), median_pool4(x).nan_to_num(7.0))


def normal_fused(d):
    """F.normalize((gx, gy, -1)) with the 2-norm sqrt(fma(gy, gy, gx * gx) + 1) in float32 (the fma via an exact float64 product)."""
    g = grad_xy(d).numpy()
    gx, gy = g[:, :1], g[:, 1:]
    s = (gy.astype(np.float64) * gy + (gx * gx).astype(np.float64)).astype(np.float32) + np.float32(1)
    nr = np.maximum(np.sqrt(s), np.float32(1e-12))
    return torch.from_numpy(np.concatenate([gx / nr, gy / nr, np.float32(-1) / nr], 1))


def _standalone(losses, t, out, c):
    seed, B, H, W, iters, k, dense, empty = c
    w = losses.loss_weights(iters)
    v, grad_gt, norm_gt = losses.gt_targets(t["flow"], t["valid"])
    seq, sm = losses.sequence_loss(out["flow_mono"], out["flow_init"], out["flow_predictions"], t["flow"], v, w)
    ini, im = losses.init_loss(out["cost_volume"], t["flow"], v, k=k, scale=0.25, threshold=0.5)
    nrm, nm = losses.disp_normal_loss(out["flow_q_predictions"], norm_gt, v, w, scale=0.25, dense_gt=bool(dense))
    grd, gm = losses.disp_grad_loss(out["disp_grad_q_predictions"], grad_gt, v, w, scale=0.25, dense_gt=bool(dense))
    for x in (seq, ini, nrm, grd):
        assert x.ndim == 0 and x.dtype == torch.float32 and x.is_cuda
    assert set(sm) == set(SEQ_KEYS) and set(im) == set(INIT_KEYS) and set(nm) == {"norm_loss"} and set(gm) == {"grad_loss"}
    return {"seq": [float(seq)] + [sm[key] for key in SEQ_KEYS], "init": [float(ini)] + [im[key] for key in INIT_KEYS],
            "norm": [float(nrm), nm["norm_loss"]], "grad": [float(grd), gm["grad_loss"]],
            "total": [float(seq) + float(ini) + 0.25 * float(nrm) + 5 * float(grd)]}


def test_each_loss_vs_golden_and_restatement(dev, gold):
    from tcs_mi355 import losses
    for i, c in _cases(gold):
        case = case_inputs(c)
        t, out = _on(case, dev, c[4])
        res = _standalone(losses, t, out, c)
        assert_matches(res, gold, i)
        assert_matches(res, {f"c{i}_{k}": np.array(v) for k, v in restate(case, c[4], c[5], bool(c[6])).items()}, i)


def test_training_objective_vs_golden(dev, gold):
    from tcs_mi355 import losses
    for i, c in _cases(gold):
        case = case_inputs(c)
        t, out = _on(case, dev, c[4])
        total, m = losses.training_objective(out, t["flow"], t["valid"], init_k=c[5], init_thres=0.5, dense_gt=bool(c[6]))
        assert list(m) == list(SEQ_KEYS) + list(INIT_KEYS) + ["norm_loss", "grad_loss"]
        res = {"seq": [np.nan] + [m[k] for k in SEQ_KEYS], "init": [m["init_loss"]] + [m[k] for k in INIT_KEYS],
               "norm": [m["norm_loss"]] * 2, "grad": [m["grad_loss"]] * 2, "total": [float(total)]}
        g = dict(gold)
        g[f"c{i}_seq"] = np.concatenate([[np.nan], gold[f"c{i}_seq"][1:]])
        assert_matches(res, g, i)
        _, vec = losses.training_objective(out, t["flow"], t["valid"], init_k=c[5], dense_gt=bool(c[6]), sync=False)
        assert vec.dtype == torch.float64 and vec.shape == (len(losses.OBJECTIVE_KEYS),)
        s = float(vec[losses.OBJECTIVE_KEYS.index("seq_loss")].cpu())
        ref = float(gold[f"c{i}_seq"][0])
        assert (np.isnan(s) and np.isnan(ref)) or abs(s - ref) <= 1e-5 * abs(ref)


def test_two_calls_bit_equal_and_stacked_equals_separate(dev, gold):
    from tcs_mi355 import losses
    i, c = _cases(gold)[1]
    t, out = _on(case_inputs(c), dev, c[4])
    a = losses.training_objective(out, t["flow"], t["valid"], init_k=c[5], dense_gt=bool(c[6]), sync=False)[1].cpu()
    b = losses.training_objective(out, t["flow"], t["valid"], init_k=c[5], dense_gt=bool(c[6]), sync=False)[1].cpu()
    assert torch.equal(a, b)
    sep = dict(out)
    sep["flow_predictions"] = [[p[0].clone(), p[1].clone()] for p in out["flow_predictions"]]
    sep["flow_q_predictions"] = [[p[0].clone(), p[1].clone()] for p in out["flow_q_predictions"]]
    sep["disp_grad_q_predictions"] = [p.clone() for p in out["disp_grad_q_predictions"]]
    assert losses._stacked_pairs(out["flow_predictions"], out["flow_mono"].shape).data_ptr() == t["up"].data_ptr()
    assert losses._stacked(out["disp_grad_q_predictions"], tuple(t["grad"].shape[1:])).data_ptr() == t["grad"].data_ptr()
    s = losses.training_objective(sep, t["flow"], t["valid"], init_k=c[5], dense_gt=bool(c[6]), sync=False)[1].cpu()
    assert torch.equal(a, s)


def test_nonfinite_prediction_raises(dev, gold):
    from tcs_mi355 import losses
    i, c = _cases(gold)[0]
    case = case_inputs(c)
    case["up"][1, 1, 0, 0, 3, 5] = np.nan
    t, out = _on(case, dev, c[4])
    with pytest.raises(FloatingPointError, match="flow prediction"):
        losses.training_objective(out, t["flow"], t["valid"])
    case = case_inputs(c)
    case["cost_volume"][0, 2, 1, 1] = np.inf
    case["grad"][0, 0, 1, 2, 3] = -np.inf
    t, out = _on(case, dev, c[4])
    with pytest.raises(FloatingPointError, match="cost volume.*gradient"):
        losses.training_objective(out, t["flow"], t["valid"])
    _, vec = losses.training_objective(out, t["flow"], t["valid"], sync=False)
    assert int(vec[-1].cpu()) == 6


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(dev, synth_weights):
    from core.tc_stereo import TCStereo
    args = Namespace(hidden_dims=[128] * 3, shared_backbone=True, corr_levels=4, corr_radius=4, n_downsample=2, context_norm="none",
                     slow_fast_gru=False, n_gru_layers=3, mixed_precision=False, init_thres=0.5)
    m = TCStereo(args)
    m.load_state_dict(synth_weights, strict=True)
    return m.to(dev).eval()


def test_end_to_end_frame(dev, model):
    """forward(test_mode=False) on the first frame of the train_outputs.npz sequence, then training_objective, against the
    restatement applied to the same outputs."""
    from tcs_mi355 import losses, synth
    seq = synth.make_sequence(7, n_frames=2, height=128, width=160, max_disp=48.0)
    fr = seq.frames[0]
    iters = 4
    im1, im2 = (torch.as_tensor(x)[None].to(dev) for x in (fr.image1, fr.image2))
    with torch.no_grad():
        o = model(im1, im2, iters=iters, test_mode=False)
    flow = -torch.as_tensor(fr.disp_gt)[None].to(dev)
    valid = (flow.abs() < 192).float()[:, 0]
    total, m = losses.training_objective(o, flow, valid, init_k=3)
    case = {"flow": flow.cpu().numpy(), "valid": valid.cpu().numpy(),
            "up": o["flow_predictions"][0][0]._base.cpu().numpy(), "q": o["flow_q_predictions"][0][0]._base.cpu().numpy(),
            "grad": o["disp_grad_q_predictions"][0]._base.cpu().numpy(), "flow_mono": o["flow_mono"].cpu().numpy(),
            "flow_init": o["flow_init"].cpu().numpy(), "cost_volume": o["cost_volume"].cpu().numpy()}
    r = restate(case, iters, 3, True)
    n = flow.numel()
    assert abs(float(total) - r["total"][0]) <= 1e-5 * abs(r["total"][0])
    for j, key in enumerate(SEQ_KEYS):
        tol = 1.0 / n if "px" in key else 1e-5 * abs(r["seq"][j + 1])
        assert abs(m[key] - r["seq"][j + 1]) <= tol, key
    for j, key in enumerate(INIT_KEYS):
        tol = 1.0 / (n // 16) if key == "forward_mask_rate" else 1e-5 * abs(r["init"][j + 1]) + 1e-7
        assert abs(m[key] - r["init"][j + 1]) <= tol, key
    assert abs(m["norm_loss"] - r["norm"][0]) <= 1e-5 * abs(r["norm"][0])
    assert abs(m["grad_loss"] - r["grad"][0]) <= 1e-5 * abs(r["grad"][0])


def test_run_sequence_objective(dev, model):
    from tcs_mi355 import synth
    from tcs_mi355.harness import run_sequence
    seq = synth.make_sequence(11, n_frames=2, height=96, width=128, max_disp=32.0)
    plain = run_sequence(model, seq, iters=3, device=dev)
    st = run_sequence(model, seq, iters=3, device=dev, objective=True)
    assert len(st.objective) == 2
    for m in st.objective:
        assert set(m) >= {"loss", "epe", "init_loss", "norm_loss", "grad_loss", "forward_mask_rate"}
        assert all(np.isfinite(v) for v in m.values()), m
    # the same predictions as test mode: the first frame bit for bit, the temporal one to the default splat's atomic-order noise
    assert st.frames[0].epe == plain.frames[0].epe
    assert abs(st.frames[1].epe - plain.frames[1].epe) <= 1e-4 * plain.frames[1].epe
