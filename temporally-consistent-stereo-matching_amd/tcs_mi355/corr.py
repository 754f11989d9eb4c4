"""`CorrBlock1D` on the HIP library: a drop-in for the reference's core/corr.py, with autograd.

Build = fp32-MFMA row GEMM + one finalize pass that pools the 4 levels, stores them in the skewed
lookup layout, and (first frame) fuses `argmax_disp`; lookup = one coalesced kernel per call instead
of 4 grid_sample chains (csrc/tcs_corr.hip).  Same constructor and methods as core/corr.py:7-79.

Gradients.  When grad mode is on and an input requires grad, the outputs carry
a gradient exactly where the reference's do.  The build is a Function of (fmap1, fmap2) whose output
is the natural level 0 volume V [B,H,W,W]; every lookup, the cost volume and `main_cost` are
Functions of V (lookups also of coords), each of whose backward returns a dense dV, so the autograd
engine sums them and a partial backward (e.g. `autograd.grad` w.r.t. coords only) stays exact.  The
skewed pyramid is saved state, not a differentiable input.  Otherwise the inference path runs as
before: same kernels, same launches, same bits.

This module imports no `core` package: the reference's training script has its own on the path.
"""
import torch
from torch.autograd.function import once_differentiable

from . import ops


def _wants_grad(*ts) -> bool:
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts)


class _CorrBuild(torch.autograd.Function):
    """(fmap1, fmap2) -> V [B,H,W,W] (corr.py:54-62).  `holder["pyr"]` receives the CorrPyramid."""

    @staticmethod
    def forward(ctx, f1, f2, holder, argmax, cost_volume):
        p = ops.corr_build(f1, f2, argmax=argmax, cost_volume=cost_volume)
        holder["pyr"] = p
        ctx.pyr = p                                   # its workspace holds V and the inverse norms
        ctx.save_for_backward(f1, f2)
        return p.workspace[: p.B * p.H * p.W * p.W].view(p.B, p.H, p.W, p.W)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_vol):
        f1, f2 = ctx.saved_tensors
        g1, g2 = ops.corr_build_backward(f1, f2, ctx.pyr, g_vol.contiguous(), ctx.needs_input_grad[0],
                                         ctx.needs_input_grad[1])
        return g1, g2, None, None, None


class _CorrLookup(torch.autograd.Function):
    """(V, coords) -> [B, 4*(2r+1), H, W] (corr.py:33-52); reads the skewed pyramid built with V."""

    @staticmethod
    def forward(ctx, vol, coords, pyr, radius):
        ctx.pyr, ctx.radius = pyr, radius
        ctx.save_for_backward(coords)
        return ops.corr_lookup(pyr, coords, radius)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        coords, = ctx.saved_tensors
        g_vol, g_coords = ops.corr_lookup_backward(ctx.pyr, coords, g.contiguous(), ctx.radius,
                                                   want_vol=ctx.needs_input_grad[0], want_coords=ctx.needs_input_grad[1])
        return g_vol, g_coords, None, None


class _CostVolume(torch.autograd.Function):
    """V -> masked cost[b,w2,h,w1] = V[b,h,w1,w2] * [w2 <= w1] (corr.py:25-31,64-65); `make()` returns the
    volume the build kernel wrote."""

    @staticmethod
    def forward(ctx, vol, make):
        return make()

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        W = g.shape[1]
        j = torch.arange(W, device=g.device)
        keep = (j.view(1, W, 1, 1) <= j.view(1, 1, 1, W))
        return torch.where(keep, g, torch.zeros((), dtype=g.dtype, device=g.device)).permute(0, 2, 3, 1).contiguous(), None


class _Argmax(torch.autograd.Function):
    """V -> (sparse_disp, main_cost, mask) (corr.py:67-79).  Only main_cost is differentiable: its gradient
    reaches the arg-max entry of the masked volume, times the 0.3-margin mask."""

    @staticmethod
    def forward(ctx, vol, make):
        sd, sc, sm = make()
        ctx.save_for_backward(sd, sm)
        ctx.mark_non_differentiable(sd, sm)
        return sd, sc, sm

    @staticmethod
    @once_differentiable
    def backward(ctx, g_disp, g_cost, g_mask):
        sd, sm = ctx.saved_tensors
        B, _, H, W = sd.shape
        g_vol = torch.zeros(B, H, W, W, dtype=torch.float32, device=sd.device)
        if g_cost is not None:
            # sparse_disp = (w1 - index) * mask: where mask = 1 the index is recovered exactly; an index in the
            # masked part (w2 > w1, value 0 there) sends no gradient to V
            w1 = torch.arange(W, device=sd.device, dtype=sd.dtype).view(1, 1, 1, W)
            idx = (w1 - sd).to(torch.int64).clamp_(0, W - 1)
            val = g_cost * sm * (sd >= 0).to(g_cost.dtype)
            g_vol.scatter_(3, idx.view(B, H, W, 1), val.reshape(B, H, W, 1).to(torch.float32))
        return g_vol, None


class CorrBlock1D:
    def __init__(self, fmap1, fmap2, num_levels=4, radius=4, thres=0.2, want_argmax=True, want_cost_volume=False):
        """`thres` is accepted and ignored like the reference (corr.py:73 hard-codes 0.3).
        want_argmax / want_cost_volume are build hints: the fused kernel emits the first-frame
        argmax and the masked [B,W2,H,W1] volume only when asked (both are recomputed on demand)."""
        if num_levels != 4:
            raise NotImplementedError("the HIP pyramid has 4 levels (corr_levels=4 in every shipped config)")
        self.num_levels, self.radius, self.thres = num_levels, radius, thres
        self._f1, self._f2 = fmap1.float().contiguous(), fmap2.float().contiguous()
        self._vol = None                      # V as an autograd tensor (grad path only)
        self._cost_t = self._sparse_t = None  # the grad path's cost volume / argmax outputs, made once
        if _wants_grad(self._f1, self._f2):
            holder = {}
            self._vol = _CorrBuild.apply(self._f1, self._f2, holder, want_argmax, want_cost_volume)
            self._pyr = holder["pyr"]
        else:
            self._pyr = ops.corr_build(self._f1, self._f2, argmax=want_argmax, cost_volume=want_cost_volume)

    def _grad_vol(self):
        return self._vol if (self._vol is not None and torch.is_grad_enabled()) else None

    def __call__(self, coords):
        """coords [B,>=1,H,W] -> [B, 4*(2r+1), H, W] float (corr.py:33-52)."""
        c = coords[:, :1].float().contiguous()
        vol = self._grad_vol()
        if vol is not None or _wants_grad(c):
            return _CorrLookup.apply(vol, c, self._pyr, self.radius)
        return ops.corr_lookup(self._pyr, c, self.radius)

    @staticmethod
    def corr(fmap1, fmap2):
        """All-pairs row correlation of the normalised maps, [B,H,W1,1,W2] (corr.py:54-62)."""
        f1, f2 = fmap1.float().contiguous(), fmap2.float().contiguous()
        if _wants_grad(f1, f2):
            v = _CorrBuild.apply(f1, f2, {}, False, False)
            B, H, W = v.shape[0], v.shape[1], v.shape[2]
            return v.reshape(B, H, W, 1, W).clone()
        p = ops.corr_build(f1, f2, natural=True)
        B, H, W = p.B, p.H, p.W
        return p.natural[0].reshape(B, H, W, 1, W).clone()

    @property
    def corr_pyramid(self):
        """Natural-layout levels [B*H*W1,1,1,W2>>i] like the reference attribute (corr.py:20-23), i=0..3."""
        vol = self._grad_vol()
        if vol is not None:
            # avg_pool2d([1,2]) chained in PyTorch from the differentiable V; same bits as the build kernel's levels
            B, H, W = self._pyr.B, self._pyr.H, self._pyr.W
            levels = [vol]
            for _ in range(3):
                v = levels[-1]
                w = v.shape[-1] // 2
                levels.append(0.5 * (v[..., 0:2 * w:2] + v[..., 1:2 * w:2]))
            return [t.reshape(B * H * W, 1, 1, -1) for t in levels]
        p = ops.corr_build(self._f1, self._f2, natural=True)
        return [t.reshape(p.B * p.H * p.W, 1, 1, -1) for t in p.natural]

    def _rebuilt(self, argmax, cost_volume):
        with torch.no_grad():
            return ops.corr_build(self._f1, self._f2, argmax=argmax, cost_volume=cost_volume)

    def get_cost_volume(self):
        vol = self._grad_vol()
        if vol is not None:
            if self._cost_t is None:
                pyr = self._pyr
                self._cost_t = _CostVolume.apply(
                    vol, lambda: pyr.cost_volume if pyr.cost_volume is not None else self._rebuilt(False, True).cost_volume)
            return self._cost_t
        if self._pyr.cost_volume is None:
            self._pyr = ops.corr_build(self._f1, self._f2, argmax=self._pyr.sparse is not None, cost_volume=True)
        return self._pyr.cost_volume

    def argmax_disp(self):
        """(sparse_disp, main_cost, mask), each [B,1,H,W] (corr.py:67-79)."""
        vol = self._grad_vol()
        if vol is not None:
            if self._sparse_t is None:
                pyr = self._pyr
                self._sparse_t = _Argmax.apply(
                    vol, lambda: pyr.sparse if pyr.sparse is not None else self._rebuilt(True, False).sparse)
            return self._sparse_t
        if self._pyr.sparse is None:
            self._pyr = ops.corr_build(self._f1, self._f2, argmax=True, cost_volume=self._pyr.cost_volume is not None)
        return self._pyr.sparse
