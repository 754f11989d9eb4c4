"""The reference's training objective (train_stereo.py:41-180, 362-399) on the MI355X: drop-in `sequence_loss`, `init_loss`,
`disp_grad_loss` and `disp_normal_loss`, plus `training_objective`, which scores a whole `TCStereo.forward(test_mode=False)` output
in five launches and one host synchronisation.

Every function returns what the reference's returns: a 0-d float32 device tensor and a dict of Python floats under the same keys.
The arithmetic is in tcs_loss.hip (per element fp32 in the reference's order, sums in fp64 finished in a fixed order, so two calls
are bit-equal).  The reference's NaN / Inf asserts become a device-side count that is read with the metrics and raised here as
FloatingPointError.  This module computes values only: inputs that require grad raise NotImplementedError (DESIGN.md sections 1,
12, 13); tcs_mi355.train_losses is the same objective with autograd, built on the plans and launches below (section 15).
Only the reference's scale 1/4 (n_downsample 2) and max_flow 700 are supported; anything else raises ValueError."""
from __future__ import annotations

from types import SimpleNamespace
from typing import Dict, List, Sequence, Tuple

import torch

from . import ops

OBJECTIVE_KEYS = ops.LOSS_KEYS        # the order of training_objective(sync=False)'s vector
SEQ_KEYS = ("epe", "epe_refine", "epe_init", "1px", "3px", "5px", "1px_refine", "3px_refine", "5px_refine")
INIT_KEYS = ("init_loss", "init_gt_loss", "init_nm_loss", "forward_mask_rate")
_IDX = {k: i for i, k in enumerate(OBJECTIVE_KEYS)}
_FLAG_TEXT = {1: "a flow prediction is NaN / Inf (or flow_init / flow_mono is NaN)", 2: "the cost volume holds NaN / Inf",
              4: "a gradient prediction is NaN / Inf"}


def loss_weights(n: int) -> List[float]:
    """train_stereo.py:362-365: gamma 0.9 adjusted to 15 / (n - 1); weight i = gamma ** (n - i - 1)."""
    n = int(n)
    if n < 2:
        raise ValueError(f"loss_weights needs at least 2 predictions (the reference divides by n - 1 = {n - 1})")
    g = 0.9 ** (15 / (n - 1))
    return [g ** (n - i - 1) for i in range(n)]


def gt_targets(flow: torch.Tensor, valid: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """train_stereo.py:367-376 at full resolution: (valid [B,1,H,W] bool, disp_grad_gt [B,2,H,W], disp_norm_gt [B,3,H,W]).
    For the standalone losses; training_objective never builds these maps (it pools straight from the flow).  Plain PyTorch
    on whatever device the inputs are on: a handful of elementwise ops, not a hot path."""
    _no_grad(flow=flow, valid=valid)
    _shape(flow, "flow", 4, c=1)
    v = valid if valid.ndim == 3 else valid[:, 0]
    mag = torch.sum(flow ** 2, dim=1).sqrt()
    vmask = ((v >= 0.5) & (mag < 700)).unsqueeze(1)
    d = torch.nn.functional.pad(-flow, (1, 1, 1, 1), mode="replicate")
    grad = torch.cat((d[:, :, 1:-1, 2:] - d[:, :, 1:-1, 1:-1], d[:, :, 2:, 1:-1] - d[:, :, 1:-1, 1:-1]), 1)
    norm = torch.nn.functional.normalize(torch.cat((grad, -torch.ones_like(grad[:, :1])), 1), dim=1)
    return vmask, grad, norm


# ---------------------------------------------------------------------------------------------
# validation
# ---------------------------------------------------------------------------------------------
def _no_grad(**tensors):
    for name, t in tensors.items():
        for x in (t if isinstance(t, (list, tuple)) else [t]):
            if isinstance(x, (list, tuple)):
                _no_grad(**{name: x})
            elif torch.is_tensor(x) and x.requires_grad:
                raise NotImplementedError(f"{name} requires grad: tcs_mi355.losses computes values only, it builds no autograd graph "
                                          f"(detach the inputs, or use tcs_mi355.train_losses, the differentiable objective)")


def _shape(t, name, ndim, c=None):
    if not torch.is_tensor(t):
        raise TypeError(f"{name}: expected a tensor, got {type(t).__name__}")
    if t.ndim != ndim or (c is not None and int(t.shape[1]) != c):
        want = f"{ndim}-D" + (f" with {c} channel(s)" if c is not None else "")
        raise ValueError(f"{name}: expected a {want} tensor, got shape {tuple(t.shape)}")


def _f32(t, name):
    if t.dtype != torch.float32:
        raise ValueError(f"{name}: expected float32, got {t.dtype}")
    return t.contiguous()


def _device(dev, **tensors):
    for name, t in tensors.items():
        if not t.is_cuda:
            raise RuntimeError(f"{name}: the MI355X objective needs HIP device tensors, got device={t.device} (there is no CPU path)")
        if t.device != dev:
            raise ValueError(f"{name} is on {t.device}, expected {dev}")


def _scale(scale):
    if abs(float(scale) - 0.25) > 0:
        raise ValueError(f"scale {scale}: the MI355X objective supports the reference's 1/4 (n_downsample 2) only")


def _valid(valid, B, H, W, name="valid"):
    """valid [B,1,H,W] or [B,H,W] -> (contiguous tensor, valid_mode): bool as bytes, anything else as float32 values."""
    if tuple(valid.shape) not in ((B, 1, H, W), (B, H, W)):
        raise ValueError(f"{name}: expected shape {(B, 1, H, W)}, got {tuple(valid.shape)}")
    if valid.dtype == torch.bool:
        return valid.contiguous(), ops.VALID_BOOL
    return valid.float().contiguous(), ops.VALID_VALUES


def _check_iters(n):
    if n < 1 or n > ops.LOSS_MAX_ITERS:
        raise ValueError(f"{n} predictions: 1 .. {ops.LOSS_MAX_ITERS} are supported")


def _weights(w, n):
    w = [float(x) for x in w]
    if len(w) < n:
        raise ValueError(f"{len(w)} loss weights for {n} predictions")
    return w[:n]


def _carries_grad(base, views) -> bool:
    """The base may stand for its views unless a view was made a leaf of its own (then only torch.stack carries its gradient)."""
    return base.requires_grad or not any(v.requires_grad for v in views)


def _stacked(entries: Sequence[torch.Tensor], shape) -> torch.Tensor:
    """The one tensor [len(entries), *shape] whose slices the entries are (forward(test_mode=False)'s lists), or a stacked copy."""
    n = len(entries)
    base = entries[0]._base
    if (base is not None and _carries_grad(base, entries) and base.is_contiguous() and base.dtype == torch.float32 and tuple(base.shape) == (n, *shape)
            and all(e._base is base and e.data_ptr() == base[i].data_ptr() and e.is_contiguous() for i, e in enumerate(entries))):
        return base
    return torch.stack([e.float() for e in entries]).contiguous()


def _stacked_pairs(pairs, shape) -> torch.Tensor:
    """[[a_0, b_0], ...] -> [n, 2, *shape], without a copy when the pairs are views of one such tensor."""
    flat = [t for p in pairs for t in p]
    if any(len(p) != 2 for p in pairs):
        raise ValueError("each prediction must be a pair [flow, flow_refine]")
    for t in flat:
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"prediction shape {tuple(t.shape)} != {tuple(shape)}")
    n = len(pairs)
    base = flat[0]._base
    if (base is not None and _carries_grad(base, flat) and base.is_contiguous() and base.dtype == torch.float32 and tuple(base.shape) == (n, 2, *shape)
            and all(t._base is base and t.data_ptr() == base[i // 2, i % 2].data_ptr() for i, t in enumerate(flat))):
        return base
    return torch.stack([torch.stack([p[0].float(), p[1].float()]) for p in pairs]).contiguous()


def _read(out: torch.Tensor) -> List[float]:
    """THE host synchronisation of a call: the fp64 output vector, with the non-finite flags raised."""
    v = out.cpu().tolist()
    flags = int(v[_IDX["nonfinite"]])
    if flags:
        why = "; ".join(t for b, t in _FLAG_TEXT.items() if flags & b)
        raise FloatingPointError(f"training objective: {why}")
    return v


# ---------------------------------------------------------------------------------------------
# plans: a validated call, as the tensors and numbers its launches need.  The public functions below and tcs_mi355.train_losses
# both build a plan and hand it to _launch, so the two modules validate and launch the same way.
# ---------------------------------------------------------------------------------------------
def _plan(parts, B, H, W, n, gt, v, mode, **kw):
    p = SimpleNamespace(parts=parts, B=B, H=H, W=W, n=n, k=1, thres=0.0, weights=None, gt=gt, v=v, vmode=mode, init_iters=1,
                        up=None, mono=None, init=None, cv=None, q=None, grad=None, targets=None, dense_gt=True,
                        grad_gt=None, grad_mask=None, grad_valid=None, norm_gt=None, norm_mask=None, norm_valid=None)
    for key, val in kw.items():
        setattr(p, key, val)
    return p


def _launch(p, counts: bool = False):
    """The launches of a plan: the quarter-resolution targets (if a quarter loss is in it), the partial sums, the finish.
    -> (out, out32) or, with counts=True, (out, out32, counts); the targets stay on the plan for the backward."""
    if p.targets == "flow":
        p.grad_gt, p.norm_gt, p.grad_mask, p.norm_mask, vdense, vsparse = ops.loss_targets(p.gt, p.v, p.vmode)
        p.grad_valid = p.norm_valid = vdense if p.dense_gt else vsparse
    elif p.targets == "full":
        pooled, gmask, vdense, vsparse = ops.loss_targets_full(p.gt, p.v, p.vmode)
        t = (pooled, gmask, vdense if p.dense_gt else vsparse)
        if p.parts == ops.LOSS_GRAD:
            p.grad_gt, p.grad_mask, p.grad_valid = t
        else:
            p.norm_gt, p.norm_mask, p.norm_valid = t
    ws = ops.loss_workspace(p.B, p.H, p.W, p.n, p.gt.device)
    if p.parts & ops.LOSS_SEQ:
        ops.sequence_loss_partials(p.up, p.gt, p.v, p.vmode, p.mono, p.init, ws)
    if p.parts & ops.LOSS_INIT:
        ops.init_loss_partials(p.cv, p.gt, p.v, p.vmode, p.k, p.thres, p.init_iters, ws)
    if p.parts & (ops.LOSS_GRAD | ops.LOSS_NORM):
        ops.grad_normal_loss_partials(p.grad, p.q, _grad_targets(p), _norm_targets(p), ws, p.H, p.W)
    return ops.loss_finish(ws, p.parts, p.B, p.H, p.W, p.n, p.k, p.weights, counts=counts)


def _grad_targets(p):
    return (p.grad_gt, p.grad_mask, p.grad_valid) if p.grad is not None else None


def _norm_targets(p):
    return (p.norm_gt, p.norm_mask, p.norm_valid) if p.q is not None else None


def _plan_sequence(flow_mono, flow_init, flow_preds, flow_gt, valid, loss_weights):
    _shape(flow_gt, "flow_gt", 4, c=1)
    B, _, H, W = (int(s) for s in flow_gt.shape)
    n = len(flow_preds)
    _check_iters(n)
    w = _weights(loss_weights, n)
    if tuple(valid.shape) != (B, 1, H, W):
        raise ValueError(f"valid shape {tuple(valid.shape)} != flow_gt shape {(B, 1, H, W)}")
    for t, name in ((flow_mono, "flow_mono"), (flow_init, "flow_init")):
        if tuple(t.shape) != (B, 1, H, W):
            raise ValueError(f"{name}: expected {(B, 1, H, W)}, got {tuple(t.shape)}")
    v, mode = _valid(valid, B, H, W)
    gt, mono, init = _f32(flow_gt, "flow_gt"), _f32(flow_mono, "flow_mono"), _f32(flow_init, "flow_init")
    _device(gt.device, valid=v, flow_mono=mono, flow_init=init, flow_preds=flow_preds[0][0])
    preds = _stacked_pairs(flow_preds, (B, 1, H, W))
    return _plan(ops.LOSS_SEQ, B, H, W, n, gt, v, mode, weights=w, up=preds, mono=mono, init=init)


def _plan_init(cost_volume, flow_gt, valid, max_flow, k, scale, threshold):
    _shape(flow_gt, "flow_gt", 4, c=1)
    _shape(cost_volume, "cost_volume", 4)
    _scale(scale)
    if float(max_flow) != 700.0:
        raise ValueError(f"max_flow {max_flow}: the MI355X objective supports the reference's 700 only")
    B, _, H, W = (int(s) for s in flow_gt.shape)
    D = int(cost_volume.shape[1])
    if tuple(cost_volume.shape) != (B, D, H // 4, W // 4):
        raise ValueError(f"cost_volume: expected [{B}, D, {H // 4}, {W // 4}], got {tuple(cost_volume.shape)}")
    k = int(k)
    if k < 1 or k > D or k > ops.LOSS_MAX_K:
        raise ValueError(f"k={k}: 1 <= k <= min({ops.LOSS_MAX_K}, D={D}) is supported")
    v, mode = _valid(valid, B, H, W)
    gt, cv = _f32(flow_gt, "flow_gt"), _f32(cost_volume, "cost_volume")
    _device(gt.device, valid=v, cost_volume=cv)
    return _plan(ops.LOSS_INIT, B, H, W, 1, gt, v, mode, k=k, thres=float(threshold), cv=cv)


def _plan_quarter(preds_stacked, gt_full, valid, loss_weights, dense_gt, part, n):
    B, Cc, H, W = (int(s) for s in gt_full.shape)
    v, mode = _valid(valid, B, H, W)
    gt = _f32(gt_full, "gt")
    _device(gt.device, valid=v, predictions=preds_stacked)
    w = _weights(loss_weights, n)
    which = {"grad": preds_stacked} if part == ops.LOSS_GRAD else {"q": preds_stacked}
    return _plan(part, B, H, W, n, gt, v, mode, weights=w, targets="full", dense_gt=bool(dense_gt), **which)


def _plan_disp_grad(disp_grad_preds, disp_grad_gt, valid, loss_weights, scale, dense_gt):
    _shape(disp_grad_gt, "disp_grad_gt", 4, c=2)
    _scale(scale)
    B, _, H, W = (int(s) for s in disp_grad_gt.shape)
    n = len(disp_grad_preds)
    _check_iters(n)
    for p in disp_grad_preds:
        if tuple(p.shape) != (B, 2, H // 4, W // 4):
            raise ValueError(f"disp_grad prediction shape {tuple(p.shape)} != {(B, 2, H // 4, W // 4)}")
    preds = _stacked(disp_grad_preds, (B, 2, H // 4, W // 4))
    return _plan_quarter(preds, disp_grad_gt, valid, loss_weights, dense_gt, ops.LOSS_GRAD, n)


def _plan_disp_normal(flow_q_preds, disp_norm_gt, valid, loss_weights, scale, dense_gt):
    _shape(disp_norm_gt, "disp_norm_gt", 4, c=3)
    _scale(scale)
    B, _, H, W = (int(s) for s in disp_norm_gt.shape)
    n = len(flow_q_preds)
    _check_iters(n)
    preds = _stacked_pairs(flow_q_preds, (B, 1, H // 4, W // 4))
    return _plan_quarter(preds, disp_norm_gt, valid, loss_weights, dense_gt, ops.LOSS_NORM, n)


_OUTPUT_KEYS = ("flow_predictions", "flow_q_predictions", "disp_grad_q_predictions", "flow_mono", "flow_init", "cost_volume")


def _output_tensors(training_output):
    missing = [k for k in _OUTPUT_KEYS if k not in training_output]
    if missing:
        raise ValueError(f"training_output lacks {missing}: call forward(..., test_mode=False)")
    return {k: training_output[k] for k in _OUTPUT_KEYS}


def _plan_objective(to, flow, valid, init_k, init_thres, n_downsample, dense_gt):
    if int(n_downsample) != 2:
        raise ValueError(f"n_downsample {n_downsample}: the MI355X objective supports the reference's 2 only")
    _shape(flow, "flow", 4, c=1)
    B, _, H, W = (int(s) for s in flow.shape)
    h, w = H // 4, W // 4
    n = len(to["flow_predictions"])
    _check_iters(n)
    wts = loss_weights(n)
    if len(to["flow_q_predictions"]) != n or len(to["disp_grad_q_predictions"]) != n:
        raise ValueError("flow_predictions, flow_q_predictions and disp_grad_q_predictions must have the same length")
    if tuple(valid.shape) not in ((B, H, W), (B, 1, H, W)):
        raise ValueError(f"valid: expected {(B, H, W)}, got {tuple(valid.shape)}")
    cv = to["cost_volume"]
    _shape(cv, "cost_volume", 4)
    D = int(cv.shape[1])
    if tuple(cv.shape) != (B, D, h, w):
        raise ValueError(f"cost_volume: expected [{B}, D, {h}, {w}], got {tuple(cv.shape)}")
    k = int(init_k)
    if k < 1 or k > D or k > ops.LOSS_MAX_K:
        raise ValueError(f"init_k={k}: 1 <= k <= min({ops.LOSS_MAX_K}, D={D}) is supported")
    for name in ("flow_mono", "flow_init"):
        if tuple(to[name].shape) != (B, 1, H, W):
            raise ValueError(f"{name}: expected {(B, 1, H, W)}, got {tuple(to[name].shape)}")
    for p in to["disp_grad_q_predictions"]:
        if tuple(p.shape) != (B, 2, h, w):
            raise ValueError(f"disp_grad prediction shape {tuple(p.shape)} != {(B, 2, h, w)}")
    gt = _f32(flow, "flow")
    v = valid.float().contiguous()
    mono, init, cv = _f32(to["flow_mono"], "flow_mono"), _f32(to["flow_init"], "flow_init"), _f32(cv, "cost_volume")
    up = _stacked_pairs(to["flow_predictions"], (B, 1, H, W))
    q = _stacked_pairs(to["flow_q_predictions"], (B, 1, h, w))
    grad = _stacked(to["disp_grad_q_predictions"], (B, 2, h, w))
    _device(gt.device, valid=v, flow_mono=mono, flow_init=init, cost_volume=cv, flow_predictions=up, flow_q_predictions=q,
            disp_grad_q_predictions=grad)
    parts = ops.LOSS_SEQ | ops.LOSS_INIT | ops.LOSS_GRAD | ops.LOSS_NORM
    return _plan(parts, B, H, W, n, gt, v, ops.VALID_TRAINER, k=k, thres=float(init_thres), weights=wts, init_iters=n, up=up,
                 mono=mono, init=init, cv=cv, q=q, grad=grad, targets="flow", dense_gt=bool(dense_gt))


# what each function returns from the finished vectors (out: float64 in OBJECTIVE_KEYS order, out32: the five losses as float32)
def _sequence_result(out, out32):
    r = _read(out)
    return out32[1], {k: r[_IDX[k]] for k in SEQ_KEYS}


def _init_result(out, out32):
    r = _read(out)
    return out32[2], {k_: r[_IDX[k_]] for k_ in INIT_KEYS}


def _disp_grad_result(out, out32, metric_name):
    r = _read(out)
    return out32[4], {metric_name: r[_IDX["grad_loss"]]}


def _disp_normal_result(out, out32, metric_name):
    r = _read(out)
    return out32[3], {metric_name: r[_IDX["norm_loss"]]}


def _objective_result(out, out32, sync):
    if not sync:
        return out32[0], out
    r = _read(out)
    metrics = {key: r[_IDX[key]] for key in SEQ_KEYS + INIT_KEYS + ("norm_loss", "grad_loss")}
    return out32[0], metrics


# ---------------------------------------------------------------------------------------------
# the reference's four losses
# ---------------------------------------------------------------------------------------------
def sequence_loss(flow_mono, flow_init, flow_preds, flow_gt, valid, loss_weights):
    """train_stereo.py:94-135: 0.1 L1(flow_init) + 0.1 L1(flow_mono) + sum_i w_i mean(|q_i - gt| + 1.2 |r_i - gt|) over the mask,
    and the EPE metrics of the last iteration."""
    _no_grad(flow_mono=flow_mono, flow_init=flow_init, flow_preds=flow_preds, flow_gt=flow_gt, valid=valid)
    return _sequence_result(*_launch(_plan_sequence(flow_mono, flow_init, flow_preds, flow_gt, valid, loss_weights)))


def init_loss(cost_volume, flow_gt, valid, max_flow=700, k=1, scale=0.25, threshold=0.1):
    """train_stereo.py:138-180 on cost_volume [B,D,H/4,W/4]: 1 - mean phi(gt) plus the hinge of the top-k zero-filled candidates
    outside [gt-1.5, gt+1.5), k <= min(8, D)."""
    _no_grad(cost_volume=cost_volume, flow_gt=flow_gt, valid=valid)
    return _init_result(*_launch(_plan_init(cost_volume, flow_gt, valid, max_flow, k, scale, threshold)))


def disp_grad_loss(disp_grad_preds, disp_grad_gt, valid, loss_weights, metric_name='grad_loss', scale=0.25, dense_gt=True):
    """train_stereo.py:41-64: the full-resolution GT gradient [B,2,H,W] median-pooled 4x4, masked |GT| < 5 and by the dense
    (max-pooled) or sparse (bilinear == 1) valid mask; sum_i w_i mean_c |pred_i - GT|."""
    _no_grad(disp_grad_preds=disp_grad_preds, disp_grad_gt=disp_grad_gt, valid=valid)
    return _disp_grad_result(*_launch(_plan_disp_grad(disp_grad_preds, disp_grad_gt, valid, loss_weights, scale, dense_gt)), metric_name)


def disp_normal_loss(flow_q_preds, disp_norm_gt, valid, loss_weights, metric_name='norm_loss', scale=0.25, dense_gt=True):
    """train_stereo.py:67-91: the full-resolution GT normal [B,3,H,W] median-pooled 4x4, masked n_x/n_z, n_y/n_z < 5; the normals
    of -flow_q and -flow_q_refine of every iteration, 0.5 mean|dn| + 0.5 (1 - n.n_gt), the refined one weighted 1.2."""
    _no_grad(flow_q_preds=flow_q_preds, disp_norm_gt=disp_norm_gt, valid=valid)
    return _disp_normal_result(*_launch(_plan_disp_normal(flow_q_preds, disp_norm_gt, valid, loss_weights, scale, dense_gt)), metric_name)


# ---------------------------------------------------------------------------------------------
# the whole objective
# ---------------------------------------------------------------------------------------------
def training_objective(training_output: Dict, flow: torch.Tensor, valid: torch.Tensor, init_k: int = 3, init_thres: float = 0.5,
                       n_downsample: int = 2, dense_gt: bool = True, sync: bool = True):
    """train_stereo.py:362-399 for one frame: `flow` [B,1,H,W] and the dataset's `valid` [B,H,W] (or [B,1,H,W]) as the trainer
    reads them; `dense_gt=False` is the trainer's kitti_raw setting.  Five launches: the quarter-resolution targets (straight
    from the flow, no full-resolution gradient), the sequence loss, the init loss, the gradient and normal losses, the finish.

    sync=True: returns (total, metrics): total = seq + init + 0.25 norm + 5 grad as a 0-d float32 device tensor, metrics the
    reference's merged dict (SEQ_KEYS, INIT_KEYS, 'norm_loss', 'grad_loss'), read with the one host synchronisation.
    sync=False: returns (total, vector) with no synchronisation: vector is a float64 device tensor in OBJECTIVE_KEYS order
    ('nonfinite' last: bit 0 flow predictions, bit 1 cost volume, bit 2 gradient predictions; not raised in this mode)."""
    to = _output_tensors(training_output)
    _no_grad(flow=flow, valid=valid, **to)
    return _objective_result(*_launch(_plan_objective(to, flow, valid, init_k, init_thres, n_downsample, dense_gt)), sync)
