"""The two non-convolution ops that carry gradient through the reference's refinement loop, with HIP forward and backward:

    from tcs_mi355 import train_ops
    import core.tc_stereo, core.update                       # the reference's own modules, on the trainer's path
    train_ops.patch_reference(core.tc_stereo, core.update)   # before the model runs

`upsample_flow(flow, mask)` is `TCStereo.upsample_flow(flow, mask, scale=True)` at n_downsample=2 (tc_stereo.py:75-88);
`upsample_flow_pair(flow_a, flow_b, mask)` is lines 213-214, `(upsample_flow(flow_a, mask.detach()), upsample_flow(flow_b, mask))`,
as one forward launch and one autograd node; `refine_blend(logits, disp_grads, disp)` is the blend at the end of
`DispRefine.forward` (update.py:294,298-300) with the candidates formed in the kernel and never written.

Each is one forward launch, bit-equal to the value-only ops (`ops.convex_upsample*`, `ops.softmax_blend` on
`ops.propagate_disparity`).  When grad mode is on and an input requires grad the output carries a grad_fn whose backward is one
launch (plus the small fixed-order gather when a flow gradient is wanted) that recomputes the softmax: the node saves the mask and
flow_b (the three inputs for the blend), nothing of the size of the softmax or the candidates.  No float atomics, no memset, no
host synchronisation; two backwards are bit-equal; a gradient that is not needed is neither computed nor allocated; double
backward raises.  Otherwise the call is the forward launch alone and no node is made.  fp16 / bf16 inputs are cast to float32
differentiably and the outputs are float32.  `disp` gets no gradient (the reference detaches it): NotImplementedError if it
requires one.  CPU tensors raise (there is no CPU path).  DESIGN.md section 16.

This module imports no `core` package: the reference's training script has its own on the path.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import ops


def _wants_grad(*ts) -> bool:
    return torch.is_grad_enabled() and any(t.requires_grad for t in ts)


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.float().contiguous()


class _Upsample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flow, mask):
        ctx.save_for_backward(flow, mask)
        return ops.upsample_flow(flow, mask)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        flow, mask = ctx.saved_tensors
        g_mask, g_flow = ops.convex_upsample_backward(flow, mask, g, want_mask=ctx.needs_input_grad[1], want_flow=ctx.needs_input_grad[0])
        return g_flow, g_mask


class _UpsamplePair(torch.autograd.Function):
    """flow_a's output reads the mask detached: the mask's gradient comes from flow_b's output alone, and flow_a is not saved (a
    flow's gradient does not depend on the flow)."""

    @staticmethod
    def forward(ctx, flow_a, flow_b, mask):
        ctx.save_for_backward(flow_b, mask)
        return ops.upsample_flow_pair(flow_a, flow_b, mask)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_a, g_b):
        flow_b, mask = ctx.saved_tensors
        need_a, need_b, need_mask = ctx.needs_input_grad
        g_mask, d_a, d_b = ops.convex_upsample_pair_backward(flow_b, mask, g_a, g_b, want_mask=need_mask, want_flow_a=need_a,
                                                             want_flow_b=need_b)
        return d_a, d_b, g_mask


class _RefineBlend(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, disp_grads, disp):
        ctx.save_for_backward(logits, disp_grads, disp)
        return ops.refine_blend(logits, disp_grads, disp)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        logits, disp_grads, disp = ctx.saved_tensors
        g_l, g_g = ops.refine_blend_backward(logits, disp_grads, disp, g, want_logits=ctx.needs_input_grad[0],
                                             want_grads=ctx.needs_input_grad[1])
        return g_l, g_g, None


def upsample_flow(flow: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """flow [N,1,H,W], mask [N,144,H,W] (channel k*16 + i*4 + j) -> [N,1,4H,4W] float32."""
    flow, mask = _f32(flow), _f32(mask)
    if _wants_grad(flow, mask):
        ops._flow_mask_dims(flow, mask)
        return _Upsample.apply(flow, mask)
    return ops.upsample_flow(flow, mask)


def upsample_flow_pair(flow_a: torch.Tensor, flow_b: torch.Tensor, mask: torch.Tensor):
    """(upsample_flow(flow_a, mask.detach()), upsample_flow(flow_b, mask)): one forward launch, one autograd node."""
    flow_a, flow_b, mask = _f32(flow_a), _f32(flow_b), _f32(mask)
    if _wants_grad(flow_a, flow_b, mask):
        ops._flow_mask_dims(flow_a, mask, "flow_a")
        ops._flow_mask_dims(flow_b, mask, "flow_b")
        return _UpsamplePair.apply(flow_a, flow_b, mask)
    return ops.upsample_flow_pair(flow_a, flow_b, mask)


def refine_blend(logits: torch.Tensor, disp_grads: torch.Tensor, disp: torch.Tensor) -> torch.Tensor:
    """logits [N,9,H,W], disp_grads [N,2,H,W], disp [N,1,H,W] -> refined disparity [N,1,H,W] float32;
    cand_k = d_n + gx_n (1-u) + gy_n (1-v), k = 3v+u, d replicate-padded and the gradient zero-padded."""
    if disp.requires_grad:
        raise NotImplementedError("disp requires grad: refine_blend is differentiable in logits and disp_grads only, the reference "
                                  "detaches the disparity (detach it)")
    logits, disp_grads, disp = _f32(logits), _f32(disp_grads), _f32(disp)
    if _wants_grad(logits, disp_grads):
        ops._blend_dims(logits, disp_grads, disp)
        return _RefineBlend.apply(logits, disp_grads, disp)
    return ops.refine_blend(logits, disp_grads, disp)


def patch_reference(tc_stereo_module, update_module):
    """Point the reference's model at these ops: `TCStereo.upsample_flow` (scale=True, one flow channel, n_downsample=2; anything else
    goes to the original) and `DispRefine.forward`, which keeps the module's own convolutions, feeds the stem from the value-only
    `ops.propagate_disparity` on detached inputs and blends with `refine_blend`.  Returns a function that undoes the patch."""
    TCStereo, DispRefine = tc_stereo_module.TCStereo, update_module.DispRefine
    originals = (TCStereo.upsample_flow, DispRefine.forward)

    def upsample(self, flow, mask, scale=True):
        if not scale or flow.shape[1] != 1 or self.args.n_downsample != 2:
            return originals[0](self, flow, mask, scale)
        return upsample_flow(flow, mask)

    def forward(self, disp_grads, disp, context_disp, context_grad, test_mode=False):
        disp = disp.detach()
        context = self.context_compress(torch.cat((context_disp, context_grad), dim=1))
        stem_in = ops.propagate_disparity(_f32(disp_grads.detach()), _f32(disp))       # 9 candidates + 18 |gradient differences|
        fused = self.conv_fuse(torch.cat((self.disp_f_stem(stem_in), context), dim=1))
        refined = refine_blend(self.w_head(fused), disp_grads, disp)
        return refined, (None if test_mode else 0.25 * self.mask(fused))

    TCStereo.upsample_flow, DispRefine.forward = upsample, forward

    def undo():
        TCStereo.upsample_flow, DispRefine.forward = originals
    return undo
