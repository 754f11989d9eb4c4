#!/usr/bin/env python3
"""Forward + backward of one ConvGRU cell's gate arithmetic (update.py:81-85, the convolutions excluded) through
tcs_mi355.train_ops.gru_reset / gru_update against the same lines in PyTorch ops, on the same GPU in the same process, the two sides
alternating rep by rep.  Inputs have the trainer's layout: z_pre / r_pre are chunk views of one [B,2C,H,W] tensor, cz / cr / cq split
views of one [B,3C,H,W] tensor; every input requires grad.  Shapes: the loop's three scales of a 320x720 crop, C = 128, B in {1, 4}.
Medians over --reps timed steps (>= 20), each ended by a device synchronise; the peak of torch.cuda.max_memory_allocated over one
forward + backward above the inputs; and, at the largest shape, each kernel alone (timed with events over 20 back-to-back launches)
against the bytes it must move and against a 16-byte-per-lane copy of the same bytes (torch's `copy_`).  One JSON line per shape.

    python tools/bench_train_gates.py [--reps 30]
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


def torch_cell(z_pre, r_pre, q0, h, cz, cr, cq):
    z = torch.sigmoid(z_pre + cz)
    r = torch.sigmoid(r_pre + cr)
    q = torch.tanh((r * h + q0) + cq)                      # r * h + q0 stands for convq(cat(r * h, x))
    return (1 - z) * h + z * q


def hip_cell(z_pre, r_pre, q0, h, cz, cr, cq):
    from tcs_mi355 import train_ops
    rh = train_ops.gru_reset(r_pre, h, cr)
    return train_ops.gru_update(z_pre, rh + q0, h, cz, cq, z_keeps_h=False)


def alternating(fns, reps):
    """Median milliseconds of each of `fns`, called in turn rep by rep, each call ended by a synchronise."""
    for _ in range(3):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[i].append((time.perf_counter() - t0) * 1e3)
    return [round(statistics.median(t), 4) for t in ts]


def peak(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def kernel_us(fn, reps, launches=20):
    """Median microseconds per launch of `fn` over `reps` event-timed bursts of `launches` back-to-back launches."""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / launches)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    assert a.reps >= 20
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from tcs_mi355 import native, ops
    native.lib()
    dev = torch.device("cuda:0")
    C = 128
    shapes = [(B, H, W) for B in (1, 4) for H, W in ((80, 180), (40, 90), (20, 45))]
    for B, H, W in shapes:
        g = torch.Generator().manual_seed(1)
        zr = (2 * torch.randn(B, 2 * C, H, W, generator=g)).to(dev).requires_grad_(True)
        ctx = torch.randn(B, 3 * C, H, W, generator=g).to(dev).requires_grad_(True)
        q0 = (2 * torch.randn(B, C, H, W, generator=g)).to(dev).requires_grad_(True)
        h = (2 * torch.rand(B, C, H, W, generator=g) - 1).to(dev).requires_grad_(True)
        up = torch.randn(B, C, H, W, generator=g).to(dev)
        leaves = [zr, ctx, q0, h]

        def step(cell):
            z_pre, r_pre = zr.chunk(2, dim=1)
            cz, cr, cq = ctx.split(C, dim=1)
            return torch.autograd.grad(cell(z_pre, r_pre, q0, h, cz, cr, cq), leaves, up)

        def fwd(cell):
            with torch.no_grad():
                return cell(*zr.chunk(2, dim=1), q0, h, *ctx.split(C, dim=1))
        res = {"shape": [B, C, H, W], "reps": a.reps, "plane_bytes": 4 * B * C * H * W}
        t = alternating([lambda: fwd(hip_cell), lambda: fwd(torch_cell), lambda: step(hip_cell), lambda: step(torch_cell)], a.reps)
        res["hip"] = {"fwd_ms": t[0], "fwd_bwd_ms": t[2], "peak_bytes": peak(lambda: step(hip_cell))}
        res["torch"] = {"fwd_ms": t[1], "fwd_bwd_ms": t[3], "peak_bytes": peak(lambda: step(torch_cell))}
        res["speedup"] = {"fwd": round(t[1] / t[0], 2), "fwd_bwd": round(t[3] / t[2], 2)}
        res["peak_saved_planes"] = round((res["torch"]["peak_bytes"] - res["hip"]["peak_bytes"]) / res["plane_bytes"], 2)
        gh, gt = step(hip_cell), step(torch_cell)
        res["max_abs_diff_over_max_grad"] = {n: float((x - y).abs().max() / y.abs().max()) for n, x, y in zip(("zr", "ctx", "q0", "h"), gh, gt)}
        if (B, H, W) == (4, 80, 180):                      # the kernels alone against the bytes they move and against a copy
            d = {k: v.detach() for k, v in zip(("z_pre", "r_pre"), zr.chunk(2, dim=1))}
            cz, cr, cq = (v.detach() for v in ctx.split(C, dim=1))
            qd, hd = q0.detach(), h.detach()
            plane = res["plane_bytes"]
            kernels = {
                "reset_fwd": (4, lambda: ops.gate_reset(d["r_pre"], hd, cr)),
                "reset_bwd": (6, lambda: ops.gate_reset_backward(d["r_pre"], hd, cr, up)),
                "update_fwd": (6, lambda: ops.gate_update(d["z_pre"], qd, hd, cz, cq, z_keeps_h=False)),
                "update_bwd": (9, lambda: ops.gate_update_backward(d["z_pre"], qd, hd, cz, cq, up, z_keeps_h=False)),
            }
            src, dst = torch.empty(3 * plane // 4, device=dev), torch.empty(3 * plane // 4, device=dev)
            copy_us = kernel_us(lambda: dst.copy_(src), a.reps)
            copy_tbs = 6 * plane / copy_us / 1e6
            res["copy"] = {"us": round(copy_us, 2), "TB_per_s": round(copy_tbs, 3)}
            res["kernels"] = {}
            for name, (planes, fn) in kernels.items():
                us = kernel_us(fn, a.reps)
                tbs = planes * plane / us / 1e6
                res["kernels"][name] = {"planes": planes, "us": round(us, 2), "TB_per_s": round(tbs, 3), "of_copy": round(tbs / copy_tbs, 3)}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
