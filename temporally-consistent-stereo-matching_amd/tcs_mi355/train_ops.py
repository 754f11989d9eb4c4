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

`gru_reset(r_pre, h, cr)` and `gru_update(z_pre, q_pre, h, cz, cq, z_keeps_h=...)` are the gate arithmetic of the recurrent cells
(update.py: ConvGRU :81-85, Lightfuse :30-34, HiddenstateUpdater :62-66) on either side of the cell's second convolution:
`r = sigmoid(r_pre + cr); rh = r * h` and `z = sigmoid(z_pre + cz); q = tanh(q_pre + cq); h_new = (1 - z) h + z q` (ConvGRU,
`z_keeps_h=False`) or `z h + (1 - z) q` (the other two, `z_keeps_h=True`; there is no default, the two differ only by the side z is
on).  One launch forward, one backward; the nodes save their inputs (the `chunk` / `split` views they were given, read in place) and
recompute z, r and q, and the gradient of a context term is the tensor of its pre-activation's gradient.
`patch_reference_cells(core.update)` points the three cells at them.  DESIGN.md section 17.

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


class _GruReset(torch.autograd.Function):
    @staticmethod
    def forward(ctx, r_pre, h, cr):
        ctx.save_for_backward(r_pre, h, cr)
        return ops.gate_reset(r_pre, h, cr)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        r_pre, h, cr = ctx.saved_tensors
        need_pre, need_h, need_cr = ctx.needs_input_grad
        g_pre, g_h = ops.gate_reset_backward(r_pre, h, cr, g, want_pre=need_pre or need_cr, want_h=need_h)
        return (g_pre if need_pre else None), g_h, (g_pre if need_cr else None)


class _GruUpdate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z_pre, q_pre, h, cz, cq, z_keeps_h):
        ctx.save_for_backward(z_pre, q_pre, h, cz, cq)
        ctx.z_keeps_h = z_keeps_h
        return ops.gate_update(z_pre, q_pre, h, cz, cq, z_keeps_h=z_keeps_h)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        z_pre, q_pre, h, cz, cq = ctx.saved_tensors
        need_z, need_q, need_h, need_cz, need_cq = ctx.needs_input_grad[:5]
        g_z, g_q, g_h = ops.gate_update_backward(z_pre, q_pre, h, cz, cq, g, z_keeps_h=ctx.z_keeps_h, want_z=need_z or need_cz,
                                                want_q=need_q or need_cq, want_h=need_h)
        return (g_z if need_z else None), (g_q if need_q else None), g_h, (g_z if need_cz else None), (g_q if need_cq else None), None


def _planes(t):
    """A gate input as the node saves it: float32 (cast differentiably), and in a layout the kernels read in place."""
    if t is None:
        return None
    if t.ndim != 4:
        raise ValueError(f"expected a 4-D NCHW tensor, got shape {tuple(t.shape)}")
    t = t.float()
    return t if ops.gate_view_ok(t) else t.contiguous()


def gru_reset(r_pre: torch.Tensor, h: torch.Tensor, cr: torch.Tensor | None = None) -> torch.Tensor:
    """sigmoid(r_pre + cr) * h, all [N,C,H,W] (cr None = zero) -> [N,C,H,W] contiguous float32."""
    r_pre, h, cr = _planes(r_pre), _planes(h), _planes(cr)
    if _wants_grad(r_pre, h, *(() if cr is None else (cr,))):
        ops._gate_dims(r_pre, "r_pre", h=h, cr=cr)
        return _GruReset.apply(r_pre, h, cr)
    return ops.gate_reset(r_pre, h, cr)


def gru_update(z_pre: torch.Tensor, q_pre: torch.Tensor, h: torch.Tensor, cz: torch.Tensor | None = None,
               cq: torch.Tensor | None = None, *, z_keeps_h: bool) -> torch.Tensor:
    """z = sigmoid(z_pre + cz), q = tanh(q_pre + cq); z_keeps_h=False: (1 - z) h + z q (ConvGRU); z_keeps_h=True: z h + (1 - z) q
    (Lightfuse, HiddenstateUpdater).  All [N,C,H,W] (cz, cq None = zero) -> [N,C,H,W] contiguous float32."""
    z_keeps_h = bool(z_keeps_h)
    z_pre, q_pre, h, cz, cq = (_planes(t) for t in (z_pre, q_pre, h, cz, cq))
    if _wants_grad(*(t for t in (z_pre, q_pre, h, cz, cq) if t is not None)):
        ops._gate_dims(z_pre, "z_pre", q_pre=q_pre, h=h, cz=cz, cq=cq)
        return _GruUpdate.apply(z_pre, q_pre, h, cz, cq, z_keeps_h)
    return ops.gate_update(z_pre, q_pre, h, cz, cq, z_keeps_h=z_keeps_h)


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


def patch_reference_cells(update_module):
    """Point the reference's recurrent cells at the gate ops: `ConvGRU.forward` (z_keeps_h=False), `Lightfuse.forward` and
    `HiddenstateUpdater.forward` (z_keeps_h=True).  Each keeps the module's own convolutions and concatenations; the reference's NaN
    asserts are dropped (they synchronise with the host).  Returns a function that undoes the patch."""
    ConvGRU, Lightfuse, Updater = update_module.ConvGRU, update_module.Lightfuse, update_module.HiddenstateUpdater
    originals = (ConvGRU.forward, Lightfuse.forward, Updater.forward)

    def gru_forward(self, h, cz, cr, cq, *x_list):
        x = torch.cat(x_list, dim=1)
        z_pre, r_pre = self.convzr(torch.cat([h, x], dim=1)).chunk(2, dim=1)
        q_pre = self.convq(torch.cat([gru_reset(r_pre, h, cr), x], dim=1))
        return gru_update(z_pre, q_pre, h, cz, cq, z_keeps_h=False)

    def fuse_forward(self, h, x):
        z_pre, r_pre = self.convzr(torch.cat([h, x], dim=1)).chunk(2, dim=1)
        q_pre = self.convq(torch.cat([gru_reset(r_pre, h), x], dim=1))
        return gru_update(z_pre, q_pre, h, z_keeps_h=True)

    def updater_forward(self, h, x):
        return fuse_forward(self, h, self.convs(x))

    ConvGRU.forward, Lightfuse.forward, Updater.forward = gru_forward, fuse_forward, updater_forward

    def undo():
        ConvGRU.forward, Lightfuse.forward, Updater.forward = originals
    return undo
