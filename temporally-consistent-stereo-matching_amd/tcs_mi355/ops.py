"""Tensor-level wrappers over the C ABI: validate, allocate outputs with torch, launch on the
current HIP stream.  One function per operator of the reference's hot path (include/tcs_mi355.h
cites the reference lines).  No arithmetic happens here."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence

import torch

from . import grouping as _grouping
from . import native as nv

ACT = {"none": 0, "relu": 1, "sigmoid": 2, "tanh": 3, "leaky": 4, "relu_add_relu": 5}
EPI_LINEAR, EPI_GRU_ZR, EPI_GRU_Q = 0, 1, 2


def _new(like: torch.Tensor, *shape) -> torch.Tensor:
    return torch.empty(shape, dtype=torch.float32, device=like.device)


def _dims4(t: torch.Tensor, name: str):
    if t.ndim != 4:
        raise ValueError(f"{name}: expected a 4-D NCHW tensor, got shape {tuple(t.shape)}")
    return tuple(int(s) for s in t.shape)


# ---------------------------------------------------------------------------------------------
# correlation
# ---------------------------------------------------------------------------------------------
@dataclass
class CorrPyramid:
    """Skewed 4-level pyramid in HBM (layout: include/tcs_mi355.h) plus what the build left behind."""
    levels: List[torch.Tensor]
    B: int
    H: int
    W: int
    workspace: torch.Tensor                       # holds the natural-layout level 0 [B,H,W,W]
    natural: Optional[List[torch.Tensor]] = None  # [B,H,W,W>>i], i = 0..3 (tests / API parity)
    cost_volume: Optional[torch.Tensor] = None    # [B,W,H,W]
    sparse: Optional[tuple] = None                # (disp, cost, mask), each [B,1,H,W]


def corr_build(fmap1: torch.Tensor, fmap2: torch.Tensor, argmax: bool = False, cost_volume: bool = False,
               natural: bool = False) -> CorrPyramid:
    B, Cc, H, W = _dims4(fmap1, "fmap1")
    if tuple(fmap2.shape) != (B, Cc, H, W):
        raise ValueError(f"fmap2 shape {tuple(fmap2.shape)} != fmap1 shape {tuple(fmap1.shape)}")
    L = nv.lib()
    ws_bytes = L.tcs_corr_build_workspace_bytes(B, H, W)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=fmap1.device)
    levels = [_new(fmap1, B, H, W >> i, W) for i in range(4)]
    nat = [None] * 4
    if natural:
        nat = [None] + [_new(fmap1, B, H, W, W >> i) for i in range(1, 4)]
    cost = _new(fmap1, B, W, H, W) if cost_volume else None
    sp = tuple(_new(fmap1, B, 1, H, W) for _ in range(3)) if argmax else (None, None, None)
    rc = L.tcs_corr_build(nv.ptr(fmap1, "fmap1"), nv.ptr(fmap2, "fmap2"), B, Cc, H, W,
                          *[nv.ptr(t) for t in levels], nv.ptr(nat[1]), nv.ptr(nat[2]), nv.ptr(nat[3]), nv.ptr(cost),
                          nv.ptr(sp[0]), nv.ptr(sp[1]), nv.ptr(sp[2]), nv.ptr(ws), nv.stream())
    nv.check(rc, "tcs_corr_build")
    out = CorrPyramid(levels, B, H, W, ws, cost_volume=cost, sparse=sp if argmax else None)
    if natural:
        out.natural = [ws[: B * H * W * W].view(B, H, W, W)] + nat[1:]
    return out


def corr_lookup(pyr: CorrPyramid, coords: torch.Tensor, radius: int = 4, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    if tuple(coords.shape) != (pyr.B, 1, pyr.H, pyr.W):
        raise ValueError(f"coords shape {tuple(coords.shape)} != {(pyr.B, 1, pyr.H, pyr.W)}")
    n_ch = 4 * (2 * radius + 1)
    if out is None:
        out = _new(coords, pyr.B, n_ch, pyr.H, pyr.W)
    elif tuple(out.shape) != (pyr.B, n_ch, pyr.H, pyr.W):
        raise ValueError("corr_lookup: bad `out` shape")
    stamps = LOOKUP_PROBE.next_slot(pyr) if LOOKUP_PROBE is not None else None
    rc = nv.lib().tcs_corr_lookup(*[nv.ptr(t) for t in pyr.levels], nv.ptr(coords, "coords"), pyr.B, pyr.H, pyr.W, radius,
                                  nv.ptr(out, "out"), stamps, nv.stream())
    nv.check(rc, "tcs_corr_lookup")
    return out


def corr_lookup_backward(pyr: CorrPyramid, coords: torch.Tensor, grad_out: torch.Tensor, radius: int = 4,
                         want_vol: bool = True, want_coords: bool = False):
    """(grad_vol [B,H,W,W] or None, grad_coords [B,1,H,W] or None) of one corr_lookup(pyr, coords, radius)."""
    B, H, W = pyr.B, pyr.H, pyr.W
    if tuple(coords.shape) != (B, 1, H, W):
        raise ValueError(f"coords shape {tuple(coords.shape)} != {(B, 1, H, W)}")
    n_ch = 4 * (2 * radius + 1)
    if tuple(grad_out.shape) != (B, n_ch, H, W):
        raise ValueError(f"grad_out shape {tuple(grad_out.shape)} != {(B, n_ch, H, W)}")
    gv = _new(coords, B, H, W, W) if want_vol else None
    gc = _new(coords, B, 1, H, W) if want_coords else None
    rc = nv.lib().tcs_corr_lookup_backward(*[nv.ptr(t) for t in pyr.levels], nv.ptr(coords, "coords"),
                                           nv.ptr(grad_out, "grad_out"), B, H, W, radius, nv.ptr(gv, "grad_vol"),
                                           nv.ptr(gc, "grad_coords"), nv.stream())
    nv.check(rc, "tcs_corr_lookup_backward")
    return gv, gc


def corr_build_backward(fmap1: torch.Tensor, fmap2: torch.Tensor, pyr: CorrPyramid, grad_vol: torch.Tensor,
                        want1: bool = True, want2: bool = True):
    """(grad_fmap1 or None, grad_fmap2 or None) of the corr_build(fmap1, fmap2) that made `pyr`, given the
    gradient of its natural level 0 volume V [B,H,W,W]."""
    B, Cc, H, W = _dims4(fmap1, "fmap1")
    if tuple(fmap2.shape) != (B, Cc, H, W):
        raise ValueError(f"fmap2 shape {tuple(fmap2.shape)} != fmap1 shape {tuple(fmap1.shape)}")
    if (pyr.B, pyr.H, pyr.W) != (B, H, W):
        raise ValueError("corr_build_backward: the pyramid was built from maps of another shape")
    if tuple(grad_vol.shape) != (B, H, W, W):
        raise ValueError(f"grad_vol shape {tuple(grad_vol.shape)} != {(B, H, W, W)}")
    L = nv.lib()
    g1 = _new(fmap1, B, Cc, H, W) if want1 else None
    g2 = _new(fmap1, B, Cc, H, W) if want2 else None
    sb = L.tcs_corr_build_backward_scratch_bytes(B, Cc, H, W)
    scratch = torch.empty(max(sb // 4, 1), dtype=torch.float32, device=fmap1.device) if sb else None
    rc = L.tcs_corr_build_backward(nv.ptr(fmap1, "fmap1"), nv.ptr(fmap2, "fmap2"), nv.ptr(pyr.workspace, "workspace"),
                                   nv.ptr(grad_vol, "grad_vol"), B, Cc, H, W, nv.ptr(g1, "grad_fmap1"),
                                   nv.ptr(g2, "grad_fmap2"), nv.ptr(scratch), nv.stream())
    nv.check(rc, "tcs_corr_build_backward")
    return g1, g2


class LookupProbe:
    """Measurement hook for bench.py: hands each lookup launch its own slot of a device buffer in
    which the kernel's workgroups record the device wall clock at start/end (include/tcs_mi355.h,
    tcs_corr_lookup `stamps`).  Works under HIP-graph capture: the slot pointer is baked into the
    captured launch, so every replay refreshes the same `slots` launches."""

    def __init__(self, device, slots: int = 64):
        self.device, self.slots, self.buf, self.blocks, self.count, self.pixels = device, slots, None, 0, 0, 0

    def next_slot(self, pyr):
        blocks = nv.lib().tcs_corr_lookup_blocks(pyr.B, pyr.H, pyr.W)
        if self.buf is None or blocks != self.blocks:
            self.blocks, self.pixels = blocks, pyr.B * pyr.H * pyr.W
            self.buf = torch.zeros(self.slots, blocks, 2, dtype=torch.int64, device=self.device)
        slot = self.count % self.slots
        self.count += 1
        return self.buf[slot].data_ptr()

    def reset(self):
        """Enqueue a clear of the stamps (end stamps are accumulated with atomicMax)."""
        if self.buf is not None:
            self.buf.zero_()

    def durations_us(self, snapshot=None):
        """Per-launch durations of the slots written since the last reset (100 MHz clock -> 10 ns ticks)."""
        buf = (self.buf if snapshot is None else snapshot).cpu()
        start, end = buf[..., 0], buf[..., 1]
        used = (end > 0).any(dim=1)
        big = torch.iinfo(torch.int64).max
        s = torch.where(start > 0, start, torch.full_like(start, big)).min(dim=1).values
        e = end.max(dim=1).values
        return ((e - s)[used].double() * 0.01).tolist()


LOOKUP_PROBE: Optional[LookupProbe] = None


def _start(start, B: int, device) -> torch.Tensor:
    """A mixed batch's sequence-start mask as the kernels take it: uint8 [B] on the device of the data (bool is converted there)."""
    if not torch.is_tensor(start) or start.ndim != 1 or int(start.shape[0]) != B or start.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f"start must be a bool / uint8 tensor of shape [{B}], got "
                         f"{tuple(start.shape) if torch.is_tensor(start) else type(start).__name__}"
                         f"{' ' + str(start.dtype) if torch.is_tensor(start) else ''}")
    if start.device != device:
        raise ValueError(f"start is on {start.device}, the data on {device}")
    return start.to(torch.uint8).contiguous()


def pose_prepare(K, T=None, T_prev=None, scale: float = 0.25, start=None):
    """-> (K_scaled, K_scaled_inv, T_rel, T_back); the last two are None without poses (tcs_pose_prepare).
    start: a mixed batch's sequence-start mask [B] (tcs_pose_prepare_mixed; needs the poses): identity T_rel / T_back for the start
    elements, whose T / T_prev are not read.  None calls tcs_pose_prepare."""
    B = int(K.shape[0])
    K = K.reshape(B, 3, 3).float().contiguous()
    ks, ksi = torch.empty_like(K), torch.empty_like(K)
    trel = tback = None
    if T is not None:
        T, T_prev = T.reshape(B, 4, 4).float().contiguous(), T_prev.reshape(B, 4, 4).float().contiguous()
        trel, tback = torch.empty_like(T), torch.empty_like(T)
    if start is not None:
        if T is None or T_prev is None:
            raise ValueError("pose_prepare(start=...) needs T and T_prev")
        start = _start(start, B, K.device)
        nv.check(nv.lib().tcs_pose_prepare_mixed(nv.ptr(K, "K"), nv.ptr(T, "T"), nv.ptr(T_prev, "previous_T"),
                                                 nv.ptr(start, "start", torch.uint8), float(scale), B, nv.ptr(ks), nv.ptr(ksi),
                                                 nv.ptr(trel), nv.ptr(tback), nv.stream()), "tcs_pose_prepare_mixed")
        return ks, ksi, trel, tback
    nv.check(nv.lib().tcs_pose_prepare(nv.ptr(K, "K"), nv.ptr(T, "T"), nv.ptr(T_prev, "previous_T"), float(scale), B,
                                       nv.ptr(ks), nv.ptr(ksi), nv.ptr(trel), nv.ptr(tback), nv.stream()), "tcs_pose_prepare")
    return ks, ksi, trel, tback


# ---------------------------------------------------------------------------------------------
# temporal warp
# ---------------------------------------------------------------------------------------------
def _cam(T_rel, K, K_inv, baseline, B):
    T_rel = T_rel.reshape(B, 4, 4).float().contiguous()
    K = K.reshape(B, 3, 3).float().contiguous()
    K_inv = K_inv.reshape(B, 3, 3).float().contiguous()
    baseline = baseline.reshape(-1).float().contiguous()
    if baseline.numel() != B:
        raise ValueError(f"baseline has {baseline.numel()} entries for batch {B}")
    return T_rel, K, K_inv, baseline


def warp_forward(prev_disp, prev_fmap, T_rel, K, K_inv, baseline, cur_fmap=None, want_fmap=True, ordered=False, start=None,
                 prior=None):
    """-> (disp [B,1,H,W], fmap [B,C,H,W] or None, mask [B,1,H,W], cost [B,1,H,W] or None)
    ordered: the splat sums in a fixed order (tcs_warp_forward_ordered), so the outputs are bit-reproducible from run to run;
    False is the float-atomic splat (tcs_warp_forward).
    start, prior: a mixed batch (tcs_warp_forward[_ordered]_mixed).  start [B] marks the elements that begin a sequence, prior is
    the first-frame prior (sparse_disp, cost, mask) [B,1,H,W] each (CorrBlock1D.argmax_disp).  A start element's disp / mask / cost
    are its prior, its fmap 0, and none of its previous-frame inputs is read; the metric mean covers the other elements only.
    None (both) calls today's entry points."""
    B, Cc, H, W = _dims4(prev_fmap, "prev_fmap")
    if tuple(prev_disp.shape) != (B, 1, H, W):
        raise ValueError("prev_disp must be [B,1,H,W] matching prev_fmap")
    if (start is None) != (prior is None):
        raise ValueError("warp_forward: start and prior go together")
    T_rel, K, K_inv, baseline = _cam(T_rel, K, K_inv, baseline, B)
    L = nv.lib()
    o_disp, o_mask = _new(prev_disp, B, 1, H, W), _new(prev_disp, B, 1, H, W)
    o_fmap = _new(prev_fmap, B, Cc, H, W) if want_fmap else None
    o_cost = _new(prev_disp, B, 1, H, W) if cur_fmap is not None else None
    ws_bytes = L.tcs_warp_ordered_workspace_bytes if ordered else L.tcs_warp_workspace_bytes
    ws = torch.empty(ws_bytes(B, Cc, H, W) // 4, dtype=torch.float32, device=prev_fmap.device)
    if start is not None:
        start = _start(start, B, prev_fmap.device)
        pr = []
        for t, nm in zip(prior, ("prior_disp", "prior_cost", "prior_mask")):
            if tuple(t.shape) != (B, 1, H, W):
                raise ValueError(f"{nm} must be [B,1,H,W] = {(B, 1, H, W)}, got {tuple(t.shape)}")
            pr.append(t.float().contiguous())
        fn, name = ((L.tcs_warp_forward_ordered_mixed, "tcs_warp_forward_ordered_mixed") if ordered else
                    (L.tcs_warp_forward_mixed, "tcs_warp_forward_mixed"))
        rc = fn(nv.ptr(prev_disp, "prev_disp"), nv.ptr(prev_fmap, "prev_fmap"), nv.ptr(T_rel), nv.ptr(K), nv.ptr(K_inv),
                nv.ptr(baseline), nv.ptr(start, "start", torch.uint8), nv.ptr(pr[0], "prior_disp"), nv.ptr(pr[1], "prior_cost"),
                nv.ptr(pr[2], "prior_mask"), B, Cc, H, W, nv.ptr(o_disp), nv.ptr(o_fmap), nv.ptr(o_mask),
                nv.ptr(cur_fmap, "cur_fmap"), nv.ptr(o_cost), nv.ptr(ws), nv.stream())
        nv.check(rc, name)
        return o_disp, o_fmap, o_mask, o_cost
    fn, name = ((L.tcs_warp_forward_ordered, "tcs_warp_forward_ordered") if ordered else (L.tcs_warp_forward, "tcs_warp_forward"))
    rc = fn(nv.ptr(prev_disp, "prev_disp"), nv.ptr(prev_fmap, "prev_fmap"), nv.ptr(T_rel), nv.ptr(K), nv.ptr(K_inv),
            nv.ptr(baseline), B, Cc, H, W, nv.ptr(o_disp), nv.ptr(o_fmap), nv.ptr(o_mask),
            nv.ptr(cur_fmap, "cur_fmap"), nv.ptr(o_cost), nv.ptr(ws), nv.stream())
    nv.check(rc, name)
    return o_disp, o_fmap, o_mask, o_cost


def warp_geometry(prev_disp, T_rel, K, K_inv, baseline):
    B, _, H, W = _dims4(prev_disp, "prev_disp")
    T_rel, K, K_inv, baseline = _cam(T_rel, K, K_inv, baseline, B)
    L = nv.lib()
    ws = torch.empty(L.tcs_warp_workspace_bytes(B, 0, H, W) // 4, dtype=torch.float32, device=prev_disp.device)
    cd, va, me = (_new(prev_disp, B, 1, H, W) for _ in range(3))
    fl = _new(prev_disp, B, 2, H, W)
    rc = L.tcs_warp_geometry(nv.ptr(prev_disp, "prev_disp"), nv.ptr(T_rel), nv.ptr(K), nv.ptr(K_inv), nv.ptr(baseline), B, H, W,
                             nv.ptr(cd), nv.ptr(va), nv.ptr(fl), nv.ptr(me), nv.ptr(ws), nv.stream())
    nv.check(rc, "tcs_warp_geometry")
    return cd, va, fl, me


def softsplat_sum(inp, flow, ordered=False):
    """Summation splat of `inp` along `flow`.  ordered: fixed summation order (tcs_softsplat_sum_ordered, bit-reproducible)."""
    B, Cc, H, W = _dims4(inp, "tenIn")
    if tuple(flow.shape) != (B, 2, H, W):
        raise ValueError("tenFlow must be [B,2,H,W]")
    if ordered:
        L = nv.lib()
        out = torch.empty_like(inp)
        ws = torch.empty(L.tcs_softsplat_ordered_workspace_bytes(B, H, W) // 4, dtype=torch.float32, device=inp.device)
        nv.check(L.tcs_softsplat_sum_ordered(nv.ptr(inp, "tenIn"), nv.ptr(flow, "tenFlow"), B, Cc, H, W, nv.ptr(out), nv.ptr(ws),
                                             nv.stream()), "tcs_softsplat_sum_ordered")
        return out
    out = torch.zeros_like(inp)
    nv.check(nv.lib().tcs_softsplat_sum(nv.ptr(inp, "tenIn"), nv.ptr(flow, "tenFlow"), B, Cc, H, W, nv.ptr(out), nv.stream()),
             "tcs_softsplat_sum")
    return out


def backward_grid(disp, T_rel, K, K_inv, baseline):
    B, _, H, W = _dims4(disp, "disp")
    T_rel, K, K_inv, baseline = _cam(T_rel, K, K_inv, baseline, B)
    grid = _new(disp, B, 2, H, W)
    nv.check(nv.lib().tcs_backward_grid(nv.ptr(disp, "disp"), nv.ptr(T_rel), nv.ptr(K), nv.ptr(K_inv), nv.ptr(baseline), B, H, W,
                                        nv.ptr(grid), nv.stream()), "tcs_backward_grid")
    return grid


def bilinear_sample(img, grid, start=None):
    """start: a mixed batch's sequence-start mask [B] (tcs_bilinear_sample_mixed): +0.0 for the start elements, whose img and grid
    are not read.  None calls tcs_bilinear_sample."""
    B, Cc, Hi, Wi = _dims4(img, "img")
    Bg, two, Ho, Wo = _dims4(grid, "grid")
    if Bg != B or two != 2:
        raise ValueError("grid must be [B,2,Ho,Wo]")
    out = _new(img, B, Cc, Ho, Wo)
    if start is not None:
        start = _start(start, B, img.device)
        nv.check(nv.lib().tcs_bilinear_sample_mixed(nv.ptr(img, "img"), nv.ptr(grid, "grid"), nv.ptr(start, "start", torch.uint8), B, Cc,
                                                    Hi, Wi, Ho, Wo, nv.ptr(out), nv.stream()), "tcs_bilinear_sample_mixed")
        return out
    nv.check(nv.lib().tcs_bilinear_sample(nv.ptr(img, "img"), nv.ptr(grid, "grid"), B, Cc, Hi, Wi, Ho, Wo, nv.ptr(out), nv.stream()),
             "tcs_bilinear_sample")
    return out


def grid_halve(grid):
    B, _, H, W = _dims4(grid, "grid")
    out = _new(grid, B, 2, H // 2, W // 2)
    nv.check(nv.lib().tcs_grid_halve(nv.ptr(grid, "grid"), B, H, W, nv.ptr(out), nv.stream()), "tcs_grid_halve")
    return out


# ---------------------------------------------------------------------------------------------
# stencils
# ---------------------------------------------------------------------------------------------
def flow_step(coords1, delta, disp_q=None):
    B, _, H, W = _dims4(coords1, "coords1")
    if disp_q is None:
        disp_q = torch.empty_like(coords1)
    nv.check(nv.lib().tcs_flow_step(nv.ptr(coords1, "coords1"), nv.ptr(delta, "delta"), B, H, W, nv.ptr(disp_q), nv.stream()),
             "tcs_flow_step")
    return disp_q


def flow_step_grads(coords1, delta, scale: float = 1.0):
    """(disp_q, scale * gradient_xy(disp_q), grad_candidates(disp_q)) with disp_q = x - (coords1 + delta), one launch."""
    B, _, H, W = _dims4(coords1, "coords1")
    if tuple(delta.shape) != (B, 1, H, W):
        raise ValueError("flow_step_grads: bad delta shape")
    disp_q, grad, cands = torch.empty_like(coords1), _new(coords1, B, 2, H, W), _new(coords1, B, 32, H, W)
    nv.check(nv.lib().tcs_flow_step_grads(nv.ptr(coords1, "coords1"), nv.ptr(delta, "delta"), B, H, W, float(scale), nv.ptr(disp_q),
                                          nv.ptr(grad), nv.ptr(cands), nv.stream()), "tcs_flow_step_grads")
    return disp_q, grad, cands


def disp_gradient_xy(disp, scale: float = 1.0, out=None):
    B, _, H, W = _dims4(disp, "disp")
    out = _new(disp, B, 2, H, W) if out is None else out
    nv.check(nv.lib().tcs_disp_gradient_xy(nv.ptr(disp, "disp"), B, H, W, float(scale), nv.ptr(out), nv.stream()), "tcs_disp_gradient_xy")
    return out


def grad_candidates(disp, out=None):
    B, _, H, W = _dims4(disp, "disp")
    out = _new(disp, B, 32, H, W) if out is None else out
    nv.check(nv.lib().tcs_grad_candidates(nv.ptr(disp, "disp"), B, H, W, nv.ptr(out), nv.stream()), "tcs_grad_candidates")
    return out


def propagate_disparity(grad, disp, out=None):
    B, _, H, W = _dims4(disp, "disp")
    out = _new(disp, B, 27, H, W) if out is None else out
    nv.check(nv.lib().tcs_propagate_disparity(nv.ptr(grad, "grad"), nv.ptr(disp, "disp"), B, H, W, nv.ptr(out), nv.stream()),
             "tcs_propagate_disparity")
    return out


def softmax_blend(logits9, cand, disp_q=None, want_delta=False, coords1=None, refined=None, flow_x=None, flow_x_channel=None):
    """`flow_x` [B,1,H,W] and `flow_x_channel` (a one-channel slice t[:, c:c+1] of a contiguous [B,C,H,W] tensor) receive
    coords1 - x, the next iteration's motion-encoder input."""
    B, _, H, W = _dims4(logits9, "logits")
    refined = _new(logits9, B, 1, H, W) if refined is None else refined
    delta = _new(logits9, B, 1, H, W) if want_delta else None
    ch_ptr, ch_stride = None, 0
    if flow_x_channel is not None:
        if tuple(flow_x_channel.shape) != (B, 1, H, W) or flow_x_channel.stride()[2:] != (W, 1) or flow_x_channel.dtype != torch.float32:
            raise ValueError("flow_x_channel must be a [B,1,H,W] float32 channel slice with dense rows")
        if not flow_x_channel.is_cuda:
            raise RuntimeError("flow_x_channel: CPU tensor (the hot path has no CPU fallback)")
        ch_ptr, ch_stride = flow_x_channel.data_ptr(), int(flow_x_channel.stride()[0]) if B > 1 else H * W
    nv.check(nv.lib().tcs_softmax_blend(nv.ptr(logits9, "logits"), nv.ptr(cand, "cand"), int(cand.shape[1]), nv.ptr(disp_q), B, H, W,
                                        nv.ptr(refined), nv.ptr(delta), nv.ptr(coords1), nv.ptr(flow_x), ch_ptr, ch_stride, nv.stream()),
             "tcs_softmax_blend")
    return refined, delta


def convex_upsample(disp, mask, clip=True):
    B, _, H, W = _dims4(disp, "disp")
    if tuple(mask.shape) != (B, 144, H, W):
        raise ValueError("mask must be [B,144,H,W] (factor 4)")
    up, fq = _new(disp, B, 1, 4 * H, 4 * W), _new(disp, B, 1, H, W)
    nv.check(nv.lib().tcs_convex_upsample(nv.ptr(disp, "disp"), nv.ptr(mask, "mask"), B, H, W, int(clip), nv.ptr(up), nv.ptr(fq), nv.stream()),
             "tcs_convex_upsample")
    return up, fq


def convex_upsample_pair(disp_a, disp_b, mask, up_a=None, up_b=None, q_a=None, q_b=None):
    """The unclipped x4 convex upsamplings of two disparities that share one mask (the two predictions of one iteration,
    tc_stereo.py:204-215) -> (up_a, up_b [B,1,4H,4W], q_a = -disp_a, q_b = -disp_b [B,1,H,W]).  Each output is bit-equal to
    `convex_upsample(disp_x, mask, clip=False)`.  Outputs may be given (contiguous float32 tensors of those shapes, e.g. slots of
    stacked per-iteration tensors); the missing ones are allocated."""
    B, _, H, W = _dims4(disp_a, "disp_a")
    if tuple(disp_b.shape) != (B, 1, H, W) or tuple(disp_a.shape) != (B, 1, H, W):
        raise ValueError("disp_a and disp_b must both be [B,1,H,W]")
    if tuple(mask.shape) != (B, 144, H, W):
        raise ValueError("mask must be [B,144,H,W] (factor 4)")
    outs = []
    for t, shape, name in ((up_a, (B, 1, 4 * H, 4 * W), "up_a"), (up_b, (B, 1, 4 * H, 4 * W), "up_b"), (q_a, (B, 1, H, W), "q_a"),
                           (q_b, (B, 1, H, W), "q_b")):
        if t is None:
            t = _new(disp_a, *shape)
        elif tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous float32 tensor of shape {shape}")
        outs.append(t)
    nv.check(nv.lib().tcs_convex_upsample_pair(nv.ptr(disp_a, "disp_a"), nv.ptr(disp_b, "disp_b"), nv.ptr(mask, "mask"), B, H, W,
                                               *(nv.ptr(t) for t in outs), nv.stream()), "tcs_convex_upsample_pair")
    return tuple(outs)


# ---------------------------------------------------------------------------------------------
# training ops: raw launches (tcs_mi355/train_ops.py holds the autograd surface)
# ---------------------------------------------------------------------------------------------
def _flow_mask_dims(flow, mask, name="flow"):
    B, D, H, W = _dims4(flow, name)
    if D != 1:
        raise ValueError(f"{name} must be [B,1,H,W], got {tuple(flow.shape)}")
    if tuple(mask.shape) != (B, 144, H, W):
        raise ValueError(f"mask must be [B,144,H,W] (factor 4) for a {name} of shape {tuple(flow.shape)}, got {tuple(mask.shape)}")
    return B, H, W


def upsample_flow(flow, mask):
    """TCStereo.upsample_flow(flow, mask, scale=True) at factor 4 -> [B,1,4H,4W]; bit-equal to convex_upsample(-flow, mask, clip=False)[0]."""
    B, H, W = _flow_mask_dims(flow, mask)
    up = _new(flow, B, 1, 4 * H, 4 * W)
    nv.check(nv.lib().tcs_upsample_flow(nv.ptr(flow, "flow"), nv.ptr(mask, "mask"), B, H, W, nv.ptr(up), nv.stream()), "tcs_upsample_flow")
    return up


def upsample_flow_pair(flow_a, flow_b, mask):
    """Both upsamplings of one iteration in one launch -> (up_a, up_b); bit-equal to convex_upsample_pair(-flow_a, -flow_b, mask)[:2]."""
    B, H, W = _flow_mask_dims(flow_a, mask, "flow_a")
    _flow_mask_dims(flow_b, mask, "flow_b")
    up_a, up_b = _new(flow_a, B, 1, 4 * H, 4 * W), _new(flow_a, B, 1, 4 * H, 4 * W)
    nv.check(nv.lib().tcs_upsample_flow_pair(nv.ptr(flow_a, "flow_a"), nv.ptr(flow_b, "flow_b"), nv.ptr(mask, "mask"), B, H, W,
                                             nv.ptr(up_a), nv.ptr(up_b), nv.stream()), "tcs_upsample_flow_pair")
    return up_a, up_b


def _grad16(g, shape, name):
    """An upstream gradient as the kernels read it: float32, contiguous, 16-byte aligned."""
    if tuple(g.shape) != shape:
        raise ValueError(f"{name} must be {shape}, got {tuple(g.shape)}")
    g = g.to(torch.float32).contiguous()
    return g.clone() if g.data_ptr() % 16 else g


def convex_upsample_pair_backward(flow_b, mask, grad_up_a, grad_up_b, want_mask=True, want_flow_a=True, want_flow_b=True):
    """Backward of upsample_flow_pair -> (grad_mask, grad_flow_a, grad_flow_b), None where not wanted (nothing is allocated for it).
    grad_mask comes from flow_b's output alone.  grad_up_a = None with want_flow_a=False is upsample_flow's backward."""
    B, H, W = _flow_mask_dims(flow_b, mask, "flow_b")
    if not (want_mask or want_flow_a or want_flow_b):
        return None, None, None
    shape = (B, 1, 4 * H, 4 * W)
    ga = _grad16(grad_up_a, shape, "grad_up_a") if want_flow_a else None
    gb = _grad16(grad_up_b, shape, "grad_up_b") if (want_mask or want_flow_b) else None
    g_mask = _new(mask, B, 144, H, W) if want_mask else None
    g_a = _new(mask, B, 1, H, W) if want_flow_a else None
    g_b = _new(mask, B, 1, H, W) if want_flow_b else None
    n = int(want_flow_a) + int(want_flow_b)
    ws = _new(mask, int(nv.lib().tcs_convex_upsample_backward_workspace_floats(B, H, W, n))) if n else None
    nv.check(nv.lib().tcs_convex_upsample_pair_backward(nv.ptr(flow_b, "flow_b"), nv.ptr(mask, "mask"), nv.ptr(ga), nv.ptr(gb), B, H, W,
                                                        nv.ptr(g_mask), nv.ptr(g_a), nv.ptr(g_b), nv.ptr(ws), nv.stream()),
             "tcs_convex_upsample_pair_backward")
    return g_mask, g_a, g_b


def convex_upsample_backward(flow, mask, grad_up, want_mask=True, want_flow=True):
    """Backward of upsample_flow -> (grad_mask, grad_flow), None where not wanted."""
    B, H, W = _flow_mask_dims(flow, mask)
    if not (want_mask or want_flow):
        return None, None
    g = _grad16(grad_up, (B, 1, 4 * H, 4 * W), "grad_up")
    g_mask = _new(mask, B, 144, H, W) if want_mask else None
    g_flow = _new(mask, B, 1, H, W) if want_flow else None
    ws = _new(mask, int(nv.lib().tcs_convex_upsample_backward_workspace_floats(B, H, W, 1))) if want_flow else None
    nv.check(nv.lib().tcs_convex_upsample_backward(nv.ptr(flow, "flow"), nv.ptr(mask, "mask"), nv.ptr(g), B, H, W, nv.ptr(g_mask),
                                                   nv.ptr(g_flow), nv.ptr(ws), nv.stream()), "tcs_convex_upsample_backward")
    return g_mask, g_flow


def _blend_dims(logits, disp_grads, disp):
    B, C, H, W = _dims4(logits, "logits")
    if C != 9:
        raise ValueError(f"logits must be [B,9,H,W], got {tuple(logits.shape)}")
    if tuple(disp_grads.shape) != (B, 2, H, W):
        raise ValueError(f"disp_grads must be {(B, 2, H, W)}, got {tuple(disp_grads.shape)}")
    if tuple(disp.shape) != (B, 1, H, W):
        raise ValueError(f"disp must be {(B, 1, H, W)}, got {tuple(disp.shape)}")
    return B, H, W


def refine_blend(logits, disp_grads, disp):
    """sum_k softmax(logits - max)_k * cand_k(disp_grads, disp) -> [B,1,H,W]; bit-equal to
    softmax_blend(logits, propagate_disparity(disp_grads, disp))[0], the candidates never written."""
    B, H, W = _blend_dims(logits, disp_grads, disp)
    refined = _new(logits, B, 1, H, W)
    nv.check(nv.lib().tcs_refine_blend(nv.ptr(logits, "logits"), nv.ptr(disp_grads, "disp_grads"), nv.ptr(disp, "disp"), B, H, W,
                                       nv.ptr(refined), nv.stream()), "tcs_refine_blend")
    return refined


def refine_blend_backward(logits, disp_grads, disp, grad_refined, want_logits=True, want_grads=True):
    """Backward of refine_blend -> (grad_logits, grad_disp_grads), None where not wanted."""
    B, H, W = _blend_dims(logits, disp_grads, disp)
    if not (want_logits or want_grads):
        return None, None
    if tuple(grad_refined.shape) != (B, 1, H, W):
        raise ValueError(f"grad_refined must be {(B, 1, H, W)}, got {tuple(grad_refined.shape)}")
    g = grad_refined.to(torch.float32).contiguous()
    g_l = _new(logits, B, 9, H, W) if want_logits else None
    g_g = _new(logits, B, 2, H, W) if want_grads else None
    nv.check(nv.lib().tcs_refine_blend_backward(nv.ptr(logits, "logits"), nv.ptr(disp_grads, "disp_grads"), nv.ptr(disp, "disp"), nv.ptr(g),
                                                B, H, W, nv.ptr(g_l), nv.ptr(g_g), nv.stream()), "tcs_refine_blend_backward")
    return g_l, g_g


def gate_view_ok(t) -> bool:
    """Whether the gate kernels read `t` [B,C,H,W] in place: contiguous planes, contiguous channels within a batch element, and a batch
    stride that steps over a whole element (what `chunk` / `split` along dim 1 of a contiguous tensor give)."""
    B, C, H, W = t.shape
    sb, sc, sh, sw = t.stride()
    inner = (W == 1 or sw == 1) and (H == 1 or sh == W) and (C == 1 or sc == H * W)
    return inner and (B == 1 or sb >= C * H * W)


def _gate_dims(first, first_name, **others):
    """[B,C,H,W] of the first tensor; ValueError unless every other one (None allowed) has the same shape."""
    shape = _dims4(first, first_name)
    for name, t in others.items():
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"{name} must be {shape} like {first_name}, got {tuple(t.shape)}")
    return shape


def _gate_in(t, name):
    """(tensor that owns the memory, device pointer, batch stride in elements) of one gate input; None -> (None, NULL, 0)."""
    if t is None:
        return None, None, 0
    if not t.is_cuda:
        raise RuntimeError(f"{name}: tcs_mi355 kernels need a HIP device tensor, got device={t.device} "
                           f"(there is no CPU path; use the oracle only for checking)")
    if t.dtype != torch.float32:
        raise ValueError(f"{name}: expected torch.float32, got {t.dtype}")
    if not gate_view_ok(t):
        t = t.contiguous()
    B, C, H, W = t.shape
    return t, t.data_ptr(), (int(t.stride(0)) if B > 1 else C * H * W)


def _gate_grad(g, shape, name):
    if tuple(g.shape) != shape:
        raise ValueError(f"{name} must be {shape}, got {tuple(g.shape)}")
    return g.to(torch.float32).contiguous()


def gate_reset(r_pre, h, cr=None):
    """sigmoid(r_pre + cr) * h -> rh [B,C,H,W] contiguous float32, one launch.  Inputs are read in place where gate_view_ok."""
    B, C, H, W = _gate_dims(r_pre, "r_pre", h=h, cr=cr)
    (k0, p_r, s_r), (k1, p_h, s_h), (k2, p_c, s_c) = _gate_in(r_pre, "r_pre"), _gate_in(h, "h"), _gate_in(cr, "cr")
    rh = _new(r_pre, B, C, H, W)
    nv.check(nv.lib().tcs_gru_reset(p_r, s_r, p_h, s_h, p_c, s_c, B, C, H, W, nv.ptr(rh), nv.stream()), "tcs_gru_reset")
    return rh


def gate_reset_backward(r_pre, h, cr, grad_rh, want_pre=True, want_h=True):
    """Backward of gate_reset -> (grad_r_pre, grad_h), None where not wanted; grad_r_pre is also the gradient of cr."""
    shape = _gate_dims(r_pre, "r_pre", h=h, cr=cr)
    if not (want_pre or want_h):
        return None, None
    B, C, H, W = shape
    (k0, p_r, s_r), (k1, p_h, s_h), (k2, p_c, s_c) = _gate_in(r_pre, "r_pre"), _gate_in(h, "h"), _gate_in(cr, "cr")
    g = _gate_grad(grad_rh, shape, "grad_rh")
    g_pre = _new(r_pre, *shape) if want_pre else None
    g_h = _new(r_pre, *shape) if want_h else None
    nv.check(nv.lib().tcs_gru_reset_backward(p_r, s_r, p_h, s_h, p_c, s_c, nv.ptr(g, "grad_rh"), B, C, H, W, nv.ptr(g_pre), nv.ptr(g_h),
                                             nv.stream()), "tcs_gru_reset_backward")
    return g_pre, g_h


def gate_update(z_pre, q_pre, h, cz=None, cq=None, *, z_keeps_h):
    """z = sigmoid(z_pre + cz), q = tanh(q_pre + cq) -> (1 - z) h + z q, or z h + (1 - z) q with z_keeps_h; one launch."""
    B, C, H, W = _gate_dims(z_pre, "z_pre", q_pre=q_pre, h=h, cz=cz, cq=cq)
    ins = [_gate_in(t, n) for t, n in ((z_pre, "z_pre"), (q_pre, "q_pre"), (h, "h"), (cz, "cz"), (cq, "cq"))]
    h_new = _new(z_pre, B, C, H, W)
    nv.check(nv.lib().tcs_gru_update(*(a for _, p, s in ins for a in (p, s)), int(bool(z_keeps_h)), B, C, H, W, nv.ptr(h_new), nv.stream()),
             "tcs_gru_update")
    return h_new


def gate_update_backward(z_pre, q_pre, h, cz, cq, grad_h_new, *, z_keeps_h, want_z=True, want_q=True, want_h=True):
    """Backward of gate_update -> (grad_z_pre, grad_q_pre, grad_h), None where not wanted; grad_z_pre is also the gradient of cz and
    grad_q_pre that of cq."""
    shape = _gate_dims(z_pre, "z_pre", q_pre=q_pre, h=h, cz=cz, cq=cq)
    if not (want_z or want_q or want_h):
        return None, None, None
    B, C, H, W = shape
    ins = [_gate_in(t, n) for t, n in ((z_pre, "z_pre"), (q_pre, "q_pre"), (h, "h"), (cz, "cz"), (cq, "cq"))]
    g = _gate_grad(grad_h_new, shape, "grad_h_new")
    g_z, g_q, g_h = (_new(z_pre, *shape) if want else None for want in (want_z, want_q, want_h))
    nv.check(nv.lib().tcs_gru_update_backward(*(a for _, p, s in ins for a in (p, s)), nv.ptr(g, "grad_h_new"), int(bool(z_keeps_h)),
                                              B, C, H, W, nv.ptr(g_z), nv.ptr(g_q), nv.ptr(g_h), nv.stream()),
             "tcs_gru_update_backward")
    return g_z, g_q, g_h


def avgpool3s2(x, out=None):
    B, Cc, H, W = _dims4(x, "x")
    out = _new(x, B, Cc, (H - 1) // 2 + 1, (W - 1) // 2 + 1) if out is None else out
    nv.check(nv.lib().tcs_avgpool3s2(nv.ptr(x, "x"), B, Cc, H, W, nv.ptr(out), nv.stream()), "tcs_avgpool3s2")
    return out


def resize_bilinear(x, Ho: int, Wo: int, out=None, scale=None):
    """Bilinear resize with align_corners=True, [B,C,H,W] -> [B,C,Ho,Wo]; `scale` (a float) multiplies the result in the same launch
    (flow_mono / flow_init: scale=-4).  scale=None is the plain resize."""
    B, Cc, H, W = _dims4(x, "x")
    out = _new(x, B, Cc, Ho, Wo) if out is None else out
    if scale is None:
        nv.check(nv.lib().tcs_resize_bilinear(nv.ptr(x, "x"), B, Cc, H, W, Ho, Wo, nv.ptr(out), nv.stream()), "tcs_resize_bilinear")
    else:
        nv.check(nv.lib().tcs_resize_bilinear_scaled(nv.ptr(x, "x"), B, Cc, H, W, Ho, Wo, float(scale), nv.ptr(out), nv.stream()),
                 "tcs_resize_bilinear_scaled")
    return out


# ---------------------------------------------------------------------------------------------
# convolutions on the matrix cores
# ---------------------------------------------------------------------------------------------
MATH_F32, MATH_F16X3 = 0, 1


@dataclass
class PackedConv:
    weight: torch.Tensor           # kernel layout (tcs_pack_conv_weight / tcs_pack_conv_weight_f16x3)
    bias: Optional[torch.Tensor]
    cout: int
    cin: int
    ksize: int
    math: int = MATH_F32
    unscale: float = 1.0
    products: int = 0              # MATH_F16X3: MFMA products per k-step (tcs_conv*_desc.products): 0 / 3 = fp16-split, 1 = fp16 only


def pack_conv(weight: torch.Tensor, bias: Optional[torch.Tensor], math: str = "f32", products: int = 0) -> PackedConv:
    """math='f32': fp32 MFMA kernel.  math='f16x3': fp16 hi/lo split kernel (fp32-equivalent accuracy);
    falls back to 'f32' for the shapes the split kernel does not cover (Cin == 1, 7x7).  `products` = 1: the f16x3 packing is
    contracted on its hi halves only (f16(x) * f16(w), fp32 accumulation; tcs_conv_desc.products); ignored by the 'f32' layout."""
    if products not in (0, 1, 3):
        raise ValueError(f"products must be 0, 1 or 3, got {products!r}")
    cout, cin, kh, kw = (int(s) for s in weight.shape)
    if kh != kw:
        raise ValueError("square kernels only")
    L = nv.lib()
    w = weight.detach().float().contiguous()
    b = None if bias is None else bias.detach().float().contiguous()
    if math == "f16x3" and cin > 1 and kh in (1, 3):
        n = L.tcs_conv_packed_floats_f16x3(cout, cin, kh)
        wmax = float(w.abs().max())
        s_log2 = 0 if wmax == 0.0 else int(12 - math_floor_log2(wmax))           # max|w| * 2^s in [2^12, 2^13)
        s_log2 = max(-40, min(40, s_log2))
        packed = torch.empty(n, dtype=torch.float32, device=w.device)
        nv.check(L.tcs_pack_conv_weight_f16x3(nv.ptr(w, "weight"), cout, cin, kh, s_log2, nv.ptr(packed), nv.stream()),
                 "tcs_pack_conv_weight_f16x3")
        return PackedConv(packed, b, cout, cin, kh, MATH_F16X3, 2.0 ** (-s_log2), int(products))
    if math not in ("f32", "f16x3"):
        raise ValueError(f"unknown math mode {math!r}")
    n = L.tcs_conv_packed_floats(cout, cin, kh)
    if n == 0:
        raise ValueError(f"unsupported convolution [{cout},{cin},{kh},{kw}]")
    packed = torch.empty(n, dtype=torch.float32, device=w.device)
    nv.check(L.tcs_pack_conv_weight(nv.ptr(w, "weight"), cout, cin, kh, nv.ptr(packed), nv.stream()), "tcs_pack_conv_weight")
    return PackedConv(packed, b, cout, cin, kh)


def pack_deconv4x4s2(weight: torch.Tensor, products: int = 0) -> PackedConv:
    """nn.ConvTranspose2d(Cin, Cout, 4, stride=2, padding=1, bias=False) -> the fp16-split layout of the equivalent
    3x3 convolution with 4*Cout parity-grouped outputs (tcs_pack_deconv4x4s2_f16x3); use with `deconv4x4s2`.  `products`: as pack_conv."""
    if products not in (0, 1, 3):
        raise ValueError(f"products must be 0, 1 or 3, got {products!r}")
    cin, cout, kh, kw = (int(s) for s in weight.shape)
    if (kh, kw) != (4, 4):
        raise ValueError("4x4 transposed convolutions only")
    L = nv.lib()
    w = weight.detach().float().contiguous()
    wmax = float(w.abs().max())
    s_log2 = 0 if wmax == 0.0 else max(-40, min(40, int(12 - math_floor_log2(wmax))))
    packed = torch.empty(L.tcs_deconv_packed_floats_f16x3(cin, cout), dtype=torch.float32, device=w.device)
    scratch = torch.empty(4 * cout * cin * 9, dtype=torch.float32, device=w.device)
    nv.check(L.tcs_pack_deconv4x4s2_f16x3(nv.ptr(w, "weight"), cin, cout, s_log2, nv.ptr(packed), nv.ptr(scratch), nv.stream()),
             "tcs_pack_deconv4x4s2_f16x3")
    return PackedConv(packed, None, 4 * cout, cin, 3, MATH_F16X3, 2.0 ** (-s_log2), int(products))


def deconv4x4s2(pc: PackedConv, srcs: Sequence[torch.Tensor], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[B,Cin,H,W] -> [B,Cout,2H,2W] (ConvTranspose2d k=4, s=2, p=1, no bias)."""
    d = _desc(pc, srcs)
    cout = pc.cout // 4
    if out is None:
        out = _new(srcs[0], d.B, cout, 2 * d.H, 2 * d.W)
    d.epilogue, d.act = 3, 0
    d.out, d.out_ctot, d.out_coff = nv.ptr(out, "out"), cout, 0
    nv.check(nv.lib().tcs_conv2d(C.byref(d), nv.stream()), "tcs_conv2d[deconv2x]")
    return out


def instance_norm(x: torch.Tensor, act: str = "none", addend: Optional[torch.Tensor] = None, eps: float = 1e-5,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(InstanceNorm2d(x)) + addend (affine=False, biased variance)."""
    B, Cc, H, W = _dims4(x, "x")
    if addend is not None and tuple(addend.shape) != (B, Cc, H, W):
        raise ValueError("instance_norm: bad addend shape")
    out = torch.empty_like(x) if out is None else out
    nv.check(nv.lib().tcs_instance_norm(nv.ptr(x, "x"), B, Cc, H, W, float(eps), ACT[act], nv.ptr(addend, "addend"), nv.ptr(out),
                                        nv.stream()), "tcs_instance_norm")
    return out


def math_floor_log2(x: float) -> int:
    import math as _m
    return int(_m.floor(_m.log2(x)))


def _desc(pc: PackedConv, srcs: Sequence[torch.Tensor]) -> nv.ConvDesc:
    if not 1 <= len(srcs) <= 4:
        raise ValueError("1..4 sources")
    B, _, H, W = _dims4(srcs[0], "src0")
    d = nv.ConvDesc()
    tot = 0
    for i, s in enumerate(srcs):
        bs, cs, hs, ws_ = _dims4(s, f"src{i}")
        if (bs, hs, ws_) != (B, H, W):
            raise ValueError(f"src{i} shape {tuple(s.shape)} does not match src0 {tuple(srcs[0].shape)}")
        d.src[i] = nv.ptr(s, f"src{i}")
        d.src_ch[i] = cs
        tot += cs
    if tot != pc.cin:
        raise ValueError(f"sources carry {tot} channels, convolution expects {pc.cin}")
    d.n_src = len(srcs)
    d.weight = nv.ptr(pc.weight)
    d.bias = nv.ptr(pc.bias)
    d.B, d.H, d.W, d.Cin, d.Cout, d.ksize = B, H, W, pc.cin, pc.cout, pc.ksize
    d.post_scale = 1.0
    d.math, d.weight_unscale = pc.math, pc.unscale
    d.products = pc.products if pc.math == MATH_F16X3 else 0
    return d


_CONV_GROUPS = _grouping.Family("ops", nv.ConvDesc, "tcs_conv2d", "tcs_conv2d_group", "tcs_conv2d_group_fused")


class grouped(_grouping.Grouped):
    """`with ops.grouped(): conv2d(...); conv2d(...)` — two INDEPENDENT tcs_conv2d layers issued as one launch at the end of the block
    where the library has a grouped kernel for them (tcs_conv2d_group), otherwise one after the other; same results either way.
    The fp32-tensor counterpart of tcs_mi355.s16.grouped (the recorder: tcs_mi355/grouping.py)."""
    family = _CONV_GROUPS


_launch_conv = _CONV_GROUPS.launch      # tcs_conv2d now, or at the end of the enclosing `grouped()` block


def conv2d(pc: PackedConv, srcs: Sequence[torch.Tensor], act: str = "none", addend=None, post_scale: float = 1.0,
           out: Optional[torch.Tensor] = None, out_coff: int = 0, stride: int = 1, out16=None, out16_group_offset: int = 0,
           image_pair: Optional[torch.Tensor] = None, in_transform: int = 0):
    """`out16` (a tcs_mi355.s16.S16): write the result in pre-split form for tcs_conv2d_s16 consumers INSTEAD of fp32 NCHW
    (returns out16); stride 1 only.  7x7 RGB stem only: `image_pair` = the right images, appended to srcs[0] along the batch
    (torch.cat((image1, image2), 0) without the copy), `in_transform=1` = samples read as 2 * (x / 255) - 1 (tc_stereo.py:101-107)."""
    d = _desc(pc, srcs)
    if image_pair is not None:
        if len(srcs) != 1 or tuple(image_pair.shape[1:]) != tuple(srcs[0].shape[1:]):
            raise ValueError("conv2d: `image_pair` must match the single source's [C,H,W]")
        d.src_batch2, d.batch_split = nv.ptr(image_pair, "image_pair"), d.B
        d.B = d.B + int(image_pair.shape[0])
    d.in_transform = int(in_transform)
    if out16 is not None:
        if stride != 1 or (out16.B, out16.H, out16.W) != (d.B, d.H, d.W):
            raise ValueError("conv2d: bad `out16`")
        if addend is not None and tuple(addend.shape) != (d.B, pc.cout, d.H, d.W):
            raise ValueError("conv2d: bad addend shape")
        d.stride = 1
        d.epilogue, d.act, d.post_scale = EPI_LINEAR, ACT[act], float(post_scale)
        d.addend = nv.ptr(addend, "addend")
        d.out16, d.out16_groups, d.out16_group_offset = out16.ptr(), out16.G, int(out16_group_offset)
        _launch_conv(d, "tcs_conv2d[s16 out]", (pc, srcs, addend, out16, image_pair))
        return out16
    if stride not in (1, 2):
        raise ValueError("stride 1 or 2")
    if stride == 2 and (pc.math != MATH_F16X3 or pc.ksize != 3):
        raise NotImplementedError("stride-2 convolutions run on the fp16-split kernel (3x3 only)")
    Ho, Wo = ((d.H - 1) // 2 + 1, (d.W - 1) // 2 + 1) if stride == 2 else (d.H, d.W)
    d.stride = stride
    if out is None:
        out = _new(srcs[0], d.B, pc.cout, Ho, Wo)
    if out.shape[0] != d.B or tuple(out.shape[2:]) != (Ho, Wo):
        raise ValueError("conv2d: bad `out` shape")
    if addend is not None and tuple(addend.shape) != (d.B, pc.cout, Ho, Wo):
        raise ValueError("conv2d: bad addend shape")
    d.epilogue, d.act, d.post_scale = EPI_LINEAR, ACT[act], float(post_scale)
    d.addend = nv.ptr(addend, "addend")
    d.out, d.out_ctot, d.out_coff = nv.ptr(out, "out"), int(out.shape[1]), int(out_coff)
    _launch_conv(d, "tcs_conv2d", (pc, srcs, addend, out, image_pair))
    return out


def conv3x3_cout1(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """Conv2d(Cin, 1, 3, padding=1) on the un-packed weight (tcs_conv3x3_cout1)."""
    B, Cin, H, W = _dims4(x, "x")
    if tuple(weight.shape) != (1, Cin, 3, 3):
        raise ValueError(f"expected a [1,{Cin},3,3] weight, got {tuple(weight.shape)}")
    out = _new(x, B, 1, H, W)
    w = weight.detach().float().contiguous()
    b = None if bias is None else bias.detach().float().contiguous()
    nv.check(nv.lib().tcs_conv3x3_cout1(nv.ptr(x, "x"), nv.ptr(w, "weight"), nv.ptr(b, "bias"), B, Cin, H, W, nv.ptr(out), nv.stream()),
             "tcs_conv3x3_cout1")
    return out


def gru_gates(pc_zr: PackedConv, srcs, h, cz=None, cr=None, z_out=None, rh_out=None):
    """z = sigmoid(conv_zr[:hid] + cz), rh = sigmoid(conv_zr[hid:] + cr) * h   (update.py:81-83, 30-33)."""
    d = _desc(pc_zr, srcs)
    hid = pc_zr.cout // 2
    if tuple(h.shape) != (d.B, hid, d.H, d.W):
        raise ValueError("gru_gates: bad h shape")
    z_out = torch.empty_like(h) if z_out is None else z_out
    rh_out = torch.empty_like(h) if rh_out is None else rh_out
    d.epilogue = EPI_GRU_ZR
    d.addend, d.addend2, d.h = nv.ptr(cz, "cz"), nv.ptr(cr, "cr"), nv.ptr(h, "h")
    d.out, d.out2, d.out_ctot, d.out_coff = nv.ptr(z_out, "z"), nv.ptr(rh_out, "rh"), hid, 0
    nv.check(nv.lib().tcs_conv2d(C.byref(d), nv.stream()), "tcs_conv2d[gru_zr]")
    return z_out, rh_out


def gru_update(pc_q: PackedConv, srcs, h, z, cq=None, keep_z: bool = False, out=None):
    """q = tanh(conv_q + cq); h' = (1-z)h + zq (keep_z=False, update.py:85) or zh + (1-z)q (update.py:34,66)."""
    d = _desc(pc_q, srcs)
    if tuple(h.shape) != (d.B, pc_q.cout, d.H, d.W) or z.shape != h.shape:
        raise ValueError("gru_update: bad h/z shape")
    out = torch.empty_like(h) if out is None else out
    d.epilogue = EPI_GRU_Q
    d.addend, d.h, d.z, d.blend_keep_z = nv.ptr(cq, "cq"), nv.ptr(h, "h"), nv.ptr(z, "z"), int(keep_z)
    d.out, d.out_ctot, d.out_coff = nv.ptr(out, "out"), pc_q.cout, 0
    nv.check(nv.lib().tcs_conv2d(C.byref(d), nv.stream()), "tcs_conv2d[gru_q]")
    return out


# ---------------------------------------------------------------------------------------------
# the training objective (tcs_loss.hip; tcs_mi355.losses is the reference-shaped surface)
# ---------------------------------------------------------------------------------------------
# the order of tcs_loss_finish's output vector (TCS_LOSS_OUT_* in include/tcs_mi355.h)
LOSS_KEYS = ("loss", "seq_loss", "init_loss", "norm_loss", "grad_loss", "epe", "epe_refine", "epe_init", "1px", "3px", "5px",
             "1px_refine", "3px_refine", "5px_refine", "init_gt_loss", "init_nm_loss", "forward_mask_rate", "nonfinite")
LOSS_SEQ, LOSS_INIT, LOSS_GRAD, LOSS_NORM = 1, 2, 4, 8
LOSS_MAX_ITERS, LOSS_MAX_K = 64, 8
VALID_VALUES, VALID_TRAINER, VALID_BOOL = 0, 1, 2      # valid_mode of the tcs_*loss* entry points
LOSS_NCOUNTS = 4                                       # TCS_LOSS_COUNT_*: seq, init, norm, grad


def _u8(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.uint8) if t.dtype == torch.bool else t


def _valid_ptr(valid: torch.Tensor, mode: int):
    return nv.ptr(_u8(valid), "valid", torch.uint8 if mode == VALID_BOOL else torch.float32)


def loss_workspace(B: int, H: int, W: int, iters: int, device) -> torch.Tensor:
    """The fp64 partial-sum buffer one objective call (any subset of the four losses) writes."""
    n = nv.lib().tcs_loss_workspace_bytes(B, H, W, iters)
    if n == 0:
        raise ValueError(f"unsupported loss shape B={B} H={H} W={W} iters={iters} (H, W >= 4; 1 <= iters <= {LOSS_MAX_ITERS})")
    return torch.empty(n // 8, dtype=torch.float64, device=device)


def loss_targets(flow_gt: torch.Tensor, valid: torch.Tensor, valid_mode: int = VALID_TRAINER):
    """flow_gt [B,1,H,W] + valid [B,(1,)H,W] -> the quarter-resolution targets of train_stereo.py:369-376 and :46-53, 72-78:
    (grad_gt [B,2,h,w], norm_gt [B,3,h,w], grad_mask, norm_mask, valid_dense, valid_sparse [B,1,h,w] bool), h = H // 4."""
    B, _, H, W = _dims4(flow_gt, "flow_gt")
    h, w = H // 4, W // 4
    dev = flow_gt.device
    grad = torch.empty(B, 2, h, w, dtype=torch.float32, device=dev)
    norm = torch.empty(B, 3, h, w, dtype=torch.float32, device=dev)
    masks = [torch.empty(B, 1, h, w, dtype=torch.bool, device=dev) for _ in range(4)]
    nv.check(nv.lib().tcs_loss_targets(nv.ptr(flow_gt, "flow_gt"), _valid_ptr(valid, valid_mode), valid_mode, B, H, W, nv.ptr(grad),
                                       nv.ptr(norm), *(nv.ptr(_u8(m), dtype=torch.uint8) for m in masks), nv.stream()), "tcs_loss_targets")
    return (grad, norm, *masks)


def loss_targets_full(gt: torch.Tensor, valid: torch.Tensor, valid_mode: int = VALID_VALUES):
    """A full-resolution GT [B,C,H,W] (C = 2 gradients, 3 normals) -> (median-pooled GT [B,C,h,w], GT mask, valid_dense, valid_sparse)."""
    B, Cc, H, W = _dims4(gt, "gt")
    h, w = H // 4, W // 4
    dev = gt.device
    out = torch.empty(B, Cc, h, w, dtype=torch.float32, device=dev)
    masks = [torch.empty(B, 1, h, w, dtype=torch.bool, device=dev) for _ in range(3)]
    nv.check(nv.lib().tcs_loss_targets_full(nv.ptr(gt, "gt"), Cc, _valid_ptr(valid, valid_mode), valid_mode, B, H, W, nv.ptr(out),
                                            *(nv.ptr(_u8(m), dtype=torch.uint8) for m in masks), nv.stream()), "tcs_loss_targets_full")
    return (out, *masks)


def sequence_loss_partials(preds: torch.Tensor, flow_gt, valid, valid_mode: int, flow_mono, flow_init, ws: torch.Tensor):
    """preds: the stacked [iters, 2, B, 1, H, W] predictions (contiguous) -> the sequence loss's partials in `ws`."""
    iters, _, B, _, H, W = (int(s) for s in preds.shape)
    n = B * H * W
    nv.check(nv.lib().tcs_sequence_loss(nv.ptr(preds, "preds"), 2 * n, n, iters, nv.ptr(flow_gt, "flow_gt"), _valid_ptr(valid, valid_mode),
                                        valid_mode, nv.ptr(flow_mono, "flow_mono"), nv.ptr(flow_init, "flow_init"), B, H, W,
                                        nv.ptr(ws, "workspace", torch.float64), nv.stream()), "tcs_sequence_loss")


def init_loss_partials(cost_volume, flow_gt, valid, valid_mode: int, k: int, threshold: float, iters: int, ws: torch.Tensor):
    B, D = int(cost_volume.shape[0]), int(cost_volume.shape[1])
    H, W = int(flow_gt.shape[2]), int(flow_gt.shape[3])
    nv.check(nv.lib().tcs_init_loss(nv.ptr(cost_volume, "cost_volume"), D, nv.ptr(flow_gt, "flow_gt"), _valid_ptr(valid, valid_mode),
                                    valid_mode, B, H, W, int(k), float(threshold), int(iters), nv.ptr(ws, "workspace", torch.float64),
                                    nv.stream()), "tcs_init_loss")


def grad_normal_loss_partials(grad_preds, q_preds, grad_t, norm_t, ws: torch.Tensor, H: int, W: int):
    """grad_preds: stacked [iters, B, 2, h, w] or None; q_preds: stacked [iters, 2, B, 1, h, w] or None;
    grad_t / norm_t: (gt, gt_mask, valid_mask) or None."""
    ref = grad_preds if grad_preds is not None else q_preds
    iters = int(ref.shape[0])
    B, h, w = int(ref.shape[-4] if grad_preds is None else ref.shape[1]), int(ref.shape[-2]), int(ref.shape[-1])
    nq = B * h * w
    g = grad_t if grad_t is not None else (None, None, None)
    m = norm_t if norm_t is not None else (None, None, None)
    u8 = torch.uint8
    nv.check(nv.lib().tcs_grad_normal_loss(nv.ptr(grad_preds, "disp_grad_preds"), 2 * nq, nv.ptr(q_preds, "flow_q_preds"), 2 * nq, nq,
                                           iters, nv.ptr(g[0], "grad_gt"), nv.ptr(_u8(g[1]) if g[1] is not None else None, dtype=u8),
                                           nv.ptr(_u8(g[2]) if g[2] is not None else None, dtype=u8), nv.ptr(m[0], "norm_gt"),
                                           nv.ptr(_u8(m[1]) if m[1] is not None else None, dtype=u8),
                                           nv.ptr(_u8(m[2]) if m[2] is not None else None, dtype=u8), B, H, W,
                                           nv.ptr(ws, "workspace", torch.float64), nv.stream()), "tcs_grad_normal_loss")


def loss_finish(ws: torch.Tensor, parts: int, B: int, H: int, W: int, iters: int, k: int, weights, counts: bool = False):
    """The partials of `parts` -> (out [len(LOSS_KEYS)] float64, out32 [5] float32: loss, seq, init, norm, grad) on the device;
    counts=True: the same launch also writes the mask counts the backward kernels divide by, (out, out32, counts [4] float64)."""
    w = (C.c_double * max(iters, 1))(*[float(x) for x in weights]) if weights is not None else None
    out = torch.empty(len(LOSS_KEYS), dtype=torch.float64, device=ws.device)
    out32 = torch.empty(5, dtype=torch.float32, device=ws.device)
    if counts:
        cnt = torch.empty(LOSS_NCOUNTS, dtype=torch.float64, device=ws.device)
        nv.check(nv.lib().tcs_loss_finish_counts(nv.ptr(ws, "workspace", torch.float64), int(parts), B, H, W, int(iters), int(k), w,
                                                 nv.ptr(out, dtype=torch.float64), nv.ptr(out32), nv.ptr(cnt, dtype=torch.float64),
                                                 nv.stream()), "tcs_loss_finish_counts")
        return out, out32, cnt
    nv.check(nv.lib().tcs_loss_finish(nv.ptr(ws, "workspace", torch.float64), int(parts), B, H, W, int(iters), int(k), w,
                                      nv.ptr(out, dtype=torch.float64), nv.ptr(out32), nv.stream()), "tcs_loss_finish")
    return out, out32


# the backward of the objective.  `counts` is loss_finish(counts=True)'s vector and `upstream` the float32 [5]
# gradient of out32, both on the device: nothing here reads them on the host.  Every returned buffer is written whole by its kernel.
def _host_weights(weights, iters: int):
    return (C.c_double * iters)(*[float(x) for x in weights[:iters]])


def _f64(t):
    return nv.ptr(t, "counts", torch.float64)


def sequence_loss_backward(preds, flow_gt, valid, valid_mode: int, flow_mono, flow_init, weights, counts, upstream,
                           want_preds: bool = True, want_mono: bool = True, want_init: bool = True):
    """-> (grad of the stacked [iters, 2, B, 1, H, W] predictions, grad flow_mono, grad flow_init); None where not wanted."""
    iters, _, B, _, H, W = (int(s) for s in preds.shape)
    n = B * H * W
    g_preds = torch.empty_like(preds) if want_preds else None
    g_mono = torch.empty_like(flow_mono) if want_mono else None
    g_init = torch.empty_like(flow_init) if want_init else None
    nv.check(nv.lib().tcs_sequence_loss_bwd(nv.ptr(preds, "preds"), 2 * n, n, iters, nv.ptr(flow_gt, "flow_gt"),
                                            _valid_ptr(valid, valid_mode), valid_mode, nv.ptr(flow_mono, "flow_mono"),
                                            nv.ptr(flow_init, "flow_init"), B, H, W, _host_weights(weights, iters), _f64(counts),
                                            nv.ptr(upstream, "upstream"), nv.ptr(g_preds), nv.ptr(g_mono), nv.ptr(g_init), nv.stream()),
             "tcs_sequence_loss_bwd")
    return g_preds, g_mono, g_init


def init_loss_backward(cost_volume, flow_gt, valid, valid_mode: int, k: int, threshold: float, counts, upstream):
    """-> the gradient of cost_volume [B,D,h,w]."""
    B, D = int(cost_volume.shape[0]), int(cost_volume.shape[1])
    H, W = int(flow_gt.shape[2]), int(flow_gt.shape[3])
    g = torch.empty_like(cost_volume)
    nv.check(nv.lib().tcs_init_loss_bwd(nv.ptr(cost_volume, "cost_volume"), D, nv.ptr(flow_gt, "flow_gt"), _valid_ptr(valid, valid_mode),
                                        valid_mode, B, H, W, int(k), float(threshold), _f64(counts), nv.ptr(upstream, "upstream"),
                                        nv.ptr(g), nv.stream()), "tcs_init_loss_bwd")
    return g


def grad_normal_loss_backward(grad_preds, q_preds, grad_t, norm_t, H: int, W: int, weights, counts, upstream):
    """grad_preds / q_preds / grad_t / norm_t as grad_normal_loss_partials (None = that loss is not differentiated)
    -> (grad of grad_preds, grad of q_preds)."""
    ref = grad_preds if grad_preds is not None else q_preds
    iters = int(ref.shape[0])
    B, h, w = int(ref.shape[-4] if grad_preds is None else ref.shape[1]), int(ref.shape[-2]), int(ref.shape[-1])
    nq = B * h * w
    g = grad_t if grad_t is not None else (None, None, None)
    m = norm_t if norm_t is not None else (None, None, None)
    u8 = torch.uint8
    g_grad = torch.empty_like(grad_preds) if grad_preds is not None else None
    g_q = torch.empty_like(q_preds) if q_preds is not None else None
    nv.check(nv.lib().tcs_grad_normal_loss_bwd(nv.ptr(grad_preds, "disp_grad_preds"), 2 * nq, nv.ptr(q_preds, "flow_q_preds"), 2 * nq, nq,
                                               iters, nv.ptr(g[0], "grad_gt"), nv.ptr(_u8(g[1]) if g[1] is not None else None, dtype=u8),
                                               nv.ptr(_u8(g[2]) if g[2] is not None else None, dtype=u8), nv.ptr(m[0], "norm_gt"),
                                               nv.ptr(_u8(m[1]) if m[1] is not None else None, dtype=u8),
                                               nv.ptr(_u8(m[2]) if m[2] is not None else None, dtype=u8), B, H, W,
                                               _host_weights(weights, iters), _f64(counts), nv.ptr(upstream, "upstream"),
                                               nv.ptr(g_grad), nv.ptr(g_q), nv.stream()), "tcs_grad_normal_loss_bwd")
    return g_grad, g_q
