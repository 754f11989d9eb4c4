#!/usr/bin/env python3
"""Forward + backward of the correlation block at the reference's training shapes (B=4; 480x640 and 320x1024 crops, features at
1/4: 120x160 and 80x256, C=256): one build, five lookups at detached coords (train_iters 5) and the masked cost volume, scored
with fixed upstream gradients.  Times, on HIP events (median of --reps), forward+backward and backward alone for
tcs_mi355.corr.CorrBlock1D and for the reference's formulation restated in PyTorch on the GPU (F.normalize, einsum, avg_pool2d,
grid_sample), plus the dense-sum cost the autograd engine pays per extra dV contribution.  One JSON line per shape.
usage: python tools/bench_corr_grad.py [--reps 20] [--warmup 5]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tcs_paths  # noqa: E402

tcs_paths.add_product_path()
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

SHAPES = [(4, 256, 120, 160), (4, 256, 80, 256)]
LOOKUPS, RADIUS = 5, 4


def torch_block(f1, f2, r=RADIUS):
    """The reference's CorrBlock1D (corr.py:8-65, utils.py:82-97) in torch ops: (lookup(coords), cost_volume)."""
    B, C, H, W = f1.shape
    vol = torch.einsum('aijk,aijh->ajkh', F.normalize(f1, dim=1), F.normalize(f2, dim=1)).reshape(B * H * W, 1, 1, W)
    pyr = [vol]
    for _ in range(3):
        pyr.append(F.avg_pool2d(pyr[-1], [1, 2], stride=[1, 2]))
    j = torch.arange(W, device=f1.device)
    cost = vol.reshape(B, H, W, W).permute(0, 3, 1, 2) * (j.view(1, W, 1, 1) <= j.view(1, 1, 1, W)).float()
    dx = torch.linspace(-r, r, 2 * r + 1, device=f1.device).view(2 * r + 1, 1)

    def lookup(coords):
        c = coords[:, :1].permute(0, 2, 3, 1).reshape(B * H * W, 1, 1, 1)
        out = []
        for i, lv in enumerate(pyr):
            x = dx + c / 2 ** i
            grid = torch.cat([2 * x / (lv.shape[-1] - 1) - 1, torch.zeros_like(x)], dim=-1)
            out.append(F.grid_sample(lv, grid, align_corners=True).view(B, H, W, -1))
        return torch.cat(out, dim=-1).permute(0, 3, 1, 2).contiguous()

    return lookup, cost


def hip_block(f1, f2):
    from tcs_mi355.corr import CorrBlock1D
    blk = CorrBlock1D(f1, f2, radius=RADIUS, want_argmax=False, want_cost_volume=True)
    return blk, blk.get_cost_volume()


def run(kind, f1, f2, coords, gl, gc):
    if kind == "hip":
        lookup, cost = hip_block(f1, f2)
    else:
        lookup, cost = torch_block(f1, f2)
    loss = (cost * gc).sum()
    for c, g in zip(coords, gl):
        loss = loss + (lookup(c) * g).sum()
    return loss


def timed(fn, reps, warmup):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for _ in range(warmup):
        fn(None)
    for e in ev:
        fn(e)
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return ms[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    from tcs_mi355 import native
    native.lib()
    for B, C, H, W in SHAPES:
        g = torch.Generator(device=dev).manual_seed(0)
        f1 = torch.randn(B, C, H, W, device=dev, generator=g).requires_grad_(True)
        f2 = torch.randn(B, C, H, W, device=dev, generator=g).requires_grad_(True)
        x = torch.arange(W, device=dev, dtype=torch.float32).view(1, 1, 1, W)
        coords = [(x - 20 * torch.rand(B, 1, H, W, device=dev, generator=g)).detach() for _ in range(LOOKUPS)]
        gl = [torch.randn(B, 4 * (2 * RADIUS + 1), H, W, device=dev, generator=g) for _ in range(LOOKUPS)]
        gc = torch.randn(B, W, H, W, device=dev, generator=g)
        res = {"shape": [B, C, H, W], "lookups": LOOKUPS, "radius": RADIUS, "reps": args.reps}
        for kind in ("hip", "torch"):
            def fwd_bwd(e):
                if e:
                    e[0].record()
                loss = run(kind, f1, f2, coords, gl, gc)
                loss.backward()
                if e:
                    e[1].record()
                f1.grad = f2.grad = None

            def bwd(e):
                loss = run(kind, f1, f2, coords, gl, gc)
                if e:
                    e[0].record()
                loss.backward()
                if e:
                    e[1].record()
                f1.grad = f2.grad = None

            res[f"{kind}_fwd_bwd_ms"] = round(timed(fwd_bwd, args.reps, args.warmup), 4)
            res[f"{kind}_bwd_ms"] = round(timed(bwd, args.reps, args.warmup), 4)
        a = torch.randn(B, H, W, W, device=dev, generator=g)
        b = torch.randn(B, H, W, W, device=dev, generator=g)

        def dense_add(e):
            if e:
                e[0].record()
            torch.add(a, b)
            if e:
                e[1].record()
        res["dV_dense_add_ms"] = round(timed(dense_add, args.reps, args.warmup), 4)
        res["dV_MB"] = round(a.numel() * 4 / 1e6, 1)
        res["speedup_fwd_bwd"] = round(res["torch_fwd_bwd_ms"] / res["hip_fwd_bwd_ms"], 2)
        res["speedup_bwd"] = round(res["torch_bwd_ms"] / res["hip_bwd_ms"], 2)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
