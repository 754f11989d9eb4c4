#!/usr/bin/env python3
"""Forward and forward + backward of tcs_mi355.train_ops.upsample_flow_pair and refine_blend against the reference's formulation of
the same two pieces in PyTorch ops (two upsample_flow calls on one mask, the second with it attached: view, max, softmax, unfold,
product, sum, permute; one-hot grouped convolutions over padded, repeated copies, then max, softmax, product, sum), on the same
GPU in the same process.  Shapes 1x120x160 and 4x80x180 (quarter resolution); medians over --reps timed steps (>= 20), each ended
by a device synchronise; the peak of torch.cuda.max_memory_allocated over one forward + backward above the inputs; and the bytes
each backward kernel must move.  Prints one JSON line per shape.

    python tools/bench_train_ops.py [--reps 30]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tcs_paths  # noqa: E402

tcs_paths.add_product_path()
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def torch_upsample_flow(flow, mask):
    N, D, H, W = flow.shape
    m = mask.view(N, 1, 9, 4, 4, H, W)
    m = torch.softmax(m - m.max(dim=2, keepdim=True)[0], dim=2)
    nb = F.unfold(4 * flow, [3, 3], padding=1).view(N, D, 9, 1, 1, H, W)
    return torch.sum(m * nb, dim=2).permute(0, 1, 4, 2, 5, 3).reshape(N, D, 4 * H, 4 * W)


def torch_upsample_flow_pair(flow_a, flow_b, mask):
    return torch_upsample_flow(flow_a, mask.detach()), torch_upsample_flow(flow_b, mask)


_ONE_HOT = {}


def torch_refine_blend(logits, disp_grads, disp):
    N, _, H, W = logits.shape
    if logits.device not in _ONE_HOT:
        k = torch.zeros(9, 1, 3, 3, device=logits.device)
        for i in range(9):
            k[i, 0, i // 3, i % 3] = 1
        cu = torch.tensor([1.0 - (i % 3) for i in range(9)], device=logits.device).view(1, 9, 1, 1)
        cv = torch.tensor([1.0 - (i // 3) for i in range(9)], device=logits.device).view(1, 9, 1, 1)
        _ONE_HOT[logits.device] = (k, cu, cv)
    k, cu, cv = _ONE_HOT[logits.device]
    x = torch.cat((F.pad(disp.detach(), (1, 1, 1, 1), mode="replicate"), F.pad(disp_grads, (1, 1, 1, 1))), dim=1)
    x = F.conv2d(x.reshape(-1, 1, H + 2, W + 2).repeat(1, 9, 1, 1), k, groups=9).reshape(N, 3, 9, H, W)
    cand = x[:, 0] + x[:, 1] * cu + x[:, 2] * cv
    w = torch.softmax(logits - logits.max(dim=1, keepdim=True)[0], dim=1)
    return torch.sum(w * cand, dim=1, keepdim=True)


def bytes_needed(B, H, W):
    """What each backward must read and write once, float32, in bytes."""
    n = 4 * B * H * W
    return {"upsample_pair_main": n * (144 + 144 + 2 * 16 + 1 + 2 * 9), "upsample_pair_gather": n * (2 * 9 + 2),
            "refine_blend": n * (9 + 2 + 1 + 1 + 9 + 2)}


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 4)


def peak(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    assert a.reps >= 20
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from tcs_mi355 import native, train_ops
    native.lib()
    dev = torch.device("cuda:0")
    for B, H, W in ((1, 120, 160), (4, 80, 180)):
        g = torch.Generator().manual_seed(1)
        fa, fb = (-(1 + 39 * torch.rand(B, 1, H, W, generator=g)).to(dev).requires_grad_(True) for _ in range(2))
        mask = (2 * torch.randn(B, 144, H, W, generator=g)).to(dev).requires_grad_(True)
        logits = (2 * torch.randn(B, 9, H, W, generator=g)).to(dev).requires_grad_(True)
        grads = (0.3 * torch.randn(B, 2, H, W, generator=g)).to(dev).requires_grad_(True)
        disp = (1 + 39 * torch.rand(B, 1, H, W, generator=g)).to(dev)
        g_a, g_b = (torch.randn(B, 1, 4 * H, 4 * W, generator=g).to(dev) for _ in range(2))
        g_r = torch.randn(B, 1, H, W, generator=g).to(dev)
        res = {"shape": [B, H, W], "reps": a.reps}
        for name, pair, blend in (("hip", train_ops.upsample_flow_pair, train_ops.refine_blend),
                                  ("torch", torch_upsample_flow_pair, torch_refine_blend)):
            def up_fwd():
                return pair(fa, fb, mask)

            def up_step():
                return torch.autograd.grad(up_fwd(), [fa, fb, mask], [g_a, g_b])

            def blend_fwd():
                return blend(logits, grads, disp)

            def blend_step():
                return torch.autograd.grad(blend_fwd(), [logits, grads], g_r)
            res[name] = {"upsample_pair_fwd_ms": timed(up_fwd, a.reps), "upsample_pair_fwd_bwd_ms": timed(up_step, a.reps),
                         "refine_blend_fwd_ms": timed(blend_fwd, a.reps), "refine_blend_fwd_bwd_ms": timed(blend_step, a.reps),
                         "upsample_pair_peak_bytes": peak(up_step), "refine_blend_peak_bytes": peak(blend_step)}
            res[name + "_grads"] = [x.clone() for x in (*up_step(), *blend_step())]
        gh, gt = res.pop("hip_grads"), res.pop("torch_grads")
        res["max_abs_diff_over_max_grad"] = {n: float((x - y).abs().max() / y.abs().max())
                                             for n, x, y in zip(("dflow_a", "dflow_b", "dmask", "dlogits", "ddisp_grads"), gh, gt)}
        res["speedup_fwd_bwd"] = {k: round(res["torch"][k + "_fwd_bwd_ms"] / res["hip"][k + "_fwd_bwd_ms"], 2)
                                  for k in ("upsample_pair", "refine_blend")}
        res["bwd_bytes"] = bytes_needed(B, H, W)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
