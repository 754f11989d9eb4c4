"""The reference's training objective (train_stereo.py:41-180, 362-399) with autograd: `tcs_mi355.losses` plus HIP backward kernels.

    from tcs_mi355.train_losses import sequence_loss, init_loss, disp_grad_loss, disp_normal_loss     # the trainer's import line
    total, metrics = training_objective(model_output, flow, valid)                                   # or the whole of lines 362-399
    scaler.scale(total / frame_length).backward()

Same signatures, return values, validation and limits as `tcs_mi355.losses` (float32, scale 1/4, max_flow 700, k <= 8).  When grad
mode is on and a prediction requires grad, the returned 0-d loss carries a grad_fn; otherwise the call is `tcs_mi355.losses`' own:
the same launches, the same bits.  Differentiable inputs: `flow_mono`, `flow_init`, every tensor of `flow_predictions`,
`flow_q_predictions` and `disp_grad_q_predictions`, and `cost_volume`, as separate tensors or as views of the stacked tensors
`TCStereo.forward(test_mode=False)` returns.  The ground truth and `valid` get no gradient: NotImplementedError if they require one.

One autograd node scores a call.  Its forward is the value-only path's launches (the finish also writes the mask counts); it saves the
inputs, the pooled targets and masks, and that count vector.  Its backward is at most three launches (csrc/tcs_loss.hip:
full-resolution maps, quarter-resolution maps, cost volume) that read the upstream gradient and the counts on the device, so there is
no host synchronisation, every gradient element is written once, and two backwards are bit-equal.  An empty mask gives a NaN loss
and all-zero gradients, as the reference's autograd does.  Double backward raises.  Ties of real values at init_loss's top-k boundary,
which torch leaves unspecified, go to the lowest candidate index.  DESIGN.md section 15.

This module imports no `core` package: the reference's training script has its own on the path.
"""
from __future__ import annotations

from typing import Dict

import torch
from torch.autograd.function import once_differentiable

from . import losses as _l
from . import ops
from .losses import OBJECTIVE_KEYS, gt_targets, loss_weights  # noqa: F401  (re-exported)

PART_KEYS = ("seq_loss", "init_loss", "norm_loss", "grad_loss")      # training_objective(return_parts=True), out32[1:5]
_INPUTS = ("up", "mono", "init", "cv", "q", "grad")                  # the plan's differentiable tensors, in apply() order


def _no_target_grad(**tensors):
    for name, t in tensors.items():
        if torch.is_tensor(t) and t.requires_grad:
            raise NotImplementedError(f"{name} requires grad: the objective is differentiable in the predictions only, the ground truth "
                                      f"and the valid mask get no gradient (detach them)")


class _Objective(torch.autograd.Function):
    """plan -> out32 [5] (total, seq, init, norm, grad; a part the plan lacks is NaN and sends no gradient) and the float64 vector."""

    @staticmethod
    def forward(ctx, plan, *inputs):
        # `inputs` are the plan's own differentiable tensors (plan.up, ...): they are arguments only so that autograd sees them; the
        # launches read them through the plan.  The plan is saved after _launch because _launch adds the pooled targets to it.
        out, out32, counts = _l._launch(plan, counts=True)
        names = [k for k, v in vars(plan).items() if torch.is_tensor(v)]
        ctx.names = names
        ctx.meta = {k: v for k, v in vars(plan).items() if not torch.is_tensor(v)}
        ctx.save_for_backward(counts, *[getattr(plan, k) for k in names])
        ctx.mark_non_differentiable(out)
        return out32, out

    @staticmethod
    @once_differentiable
    def backward(ctx, g32, _g_out):
        counts, *saved = ctx.saved_tensors
        t = dict(zip(ctx.names, saved))
        m = ctx.meta
        get = t.get
        need = dict(zip(_INPUTS, ctx.needs_input_grad[1:]))
        up = g32.to(torch.float32).contiguous()
        g = dict.fromkeys(_INPUTS)
        w = m["weights"]
        if m["parts"] & ops.LOSS_SEQ and (need["up"] or need["mono"] or need["init"]):
            g["up"], g["mono"], g["init"] = ops.sequence_loss_backward(t["up"], t["gt"], t["v"], m["vmode"], t["mono"], t["init"], w,
                                                                       counts, up, need["up"], need["mono"], need["init"])
        if m["parts"] & ops.LOSS_INIT and need["cv"]:
            g["cv"] = ops.init_loss_backward(t["cv"], t["gt"], t["v"], m["vmode"], m["k"], m["thres"], counts, up)
        want_grad = bool(m["parts"] & ops.LOSS_GRAD) and need["grad"]
        want_q = bool(m["parts"] & ops.LOSS_NORM) and need["q"]
        if want_grad or want_q:
            g["grad"], g["q"] = ops.grad_normal_loss_backward(
                t["grad"] if want_grad else None, t["q"] if want_q else None,
                (get("grad_gt"), get("grad_mask"), get("grad_valid")) if want_grad else None,
                (get("norm_gt"), get("norm_mask"), get("norm_valid")) if want_q else None, m["H"], m["W"], w, counts, up)
        return (None, *[g[k] for k in _INPUTS])


def _score(plan):
    """(out, out32) of a plan: through the autograd node when a prediction wants a gradient, else losses' own launches."""
    inputs = [getattr(plan, k) for k in _INPUTS]
    if torch.is_grad_enabled() and any(x is not None and x.requires_grad for x in inputs):
        out32, out = _Objective.apply(plan, *inputs)
        return out, out32
    return _l._launch(plan)


def sequence_loss(flow_mono, flow_init, flow_preds, flow_gt, valid, loss_weights):
    """losses.sequence_loss, differentiable in flow_mono, flow_init and every tensor of flow_preds."""
    _no_target_grad(flow_gt=flow_gt, valid=valid)
    return _l._sequence_result(*_score(_l._plan_sequence(flow_mono, flow_init, flow_preds, flow_gt, valid, loss_weights)))


def init_loss(cost_volume, flow_gt, valid, max_flow=700, k=1, scale=0.25, threshold=0.1):
    """losses.init_loss, differentiable in cost_volume (phi_gt is detached inside the hinge, as in the reference)."""
    _no_target_grad(flow_gt=flow_gt, valid=valid)
    return _l._init_result(*_score(_l._plan_init(cost_volume, flow_gt, valid, max_flow, k, scale, threshold)))


def disp_grad_loss(disp_grad_preds, disp_grad_gt, valid, loss_weights, metric_name='grad_loss', scale=0.25, dense_gt=True):
    """losses.disp_grad_loss, differentiable in every tensor of disp_grad_preds."""
    _no_target_grad(disp_grad_gt=disp_grad_gt, valid=valid)
    return _l._disp_grad_result(*_score(_l._plan_disp_grad(disp_grad_preds, disp_grad_gt, valid, loss_weights, scale, dense_gt)),
                                metric_name)


def disp_normal_loss(flow_q_preds, disp_norm_gt, valid, loss_weights, metric_name='norm_loss', scale=0.25, dense_gt=True):
    """losses.disp_normal_loss, differentiable in every tensor of flow_q_preds."""
    _no_target_grad(disp_norm_gt=disp_norm_gt, valid=valid)
    return _l._disp_normal_result(*_score(_l._plan_disp_normal(flow_q_preds, disp_norm_gt, valid, loss_weights, scale, dense_gt)),
                                  metric_name)


def training_objective(training_output: Dict, flow: torch.Tensor, valid: torch.Tensor, init_k: int = 3, init_thres: float = 0.5,
                       n_downsample: int = 2, dense_gt: bool = True, sync: bool = True, return_parts: bool = False):
    """losses.training_objective with a differentiable `total`.  sync=True still reads the metrics with the forward's one host
    synchronisation; sync=False makes none (backward never does).

    return_parts=True appends a third value, {'seq_loss', 'init_loss', 'norm_loss', 'grad_loss'} as 0-d float32 device tensors
    of the same autograd node as `total` (= seq + init + 0.25 norm + 5 grad), for a trainer that weights the parts itself: any
    combination of them and `total` backpropagates in one pass of the same three launches."""
    to = _l._output_tensors(training_output)
    _no_target_grad(flow=flow, valid=valid)
    out, out32 = _score(_l._plan_objective(to, flow, valid, init_k, init_thres, n_downsample, dense_gt))
    res = _l._objective_result(out, out32, sync)
    if return_parts:
        return (*res, {key: out32[1 + i] for i, key in enumerate(PART_KEYS)})
    return res
