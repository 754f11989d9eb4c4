#!/usr/bin/env python3
"""Forward + backward of the training objective per frame: tcs_mi355.train_losses.training_objective(sync=False) and .backward()
(the HIP forward launches, at most three backward launches, no host synchronisation) against the same objective in PyTorch ops
(tools/bench_losses.torch_objective: the trainer's ATen ops, phi_gt detached in the hinge, and its .item() per metric) with .backward(), on the same GPU in the same
process.  Shapes: 640x480 at B = 1 and the trainer's crop 320x720 at B = 4; medians over --reps timed steps (>= 20), each step
ended by a device synchronise.  Also the device time of the HIP backward alone (events around --reps backwards of retained graphs)
and the bytes each backward kernel must move.  Prints one JSON line per shape and iteration count.

    python tools/bench_loss_grad.py [--iters 5 32] [--reps 30]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import tcs_paths  # noqa: E402

tcs_paths.add_product_path()
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bench_losses import torch_objective  # noqa: E402

LEAVES = ("up", "q", "grad", "flow_mono", "flow_init", "cost_volume")


def bytes_needed(B, H, W, iters):
    """What each backward kernel must read and write once (float32 maps; masks and targets included), in bytes."""
    n, nq, D = B * H * W, B * (H // 4) * (W // 4), W // 4
    full = 4 * n * (2 + 2 * (2 * iters + 2))                       # gt, valid; every map read and its gradient written
    quarter = nq * (4 * 2 * (2 * iters + 2 * iters) + 4 * 5 + 4)   # grad (2 ch) and q pairs in + out; 5 target floats, 4 mask bytes
    volume = 4 * nq * D * 2 + 8 * nq
    return {"full": full, "quarter": quarter, "volume": volume}


def as_output(leaf, iters):
    """The stacked leaves as the model's training-output dict (the lists are views of them)."""
    return {"flow_predictions": [[leaf["up"][i, 0], leaf["up"][i, 1]] for i in range(iters)],
            "flow_q_predictions": [[leaf["q"][i, 0], leaf["q"][i, 1]] for i in range(iters)],
            "disp_grad_q_predictions": [leaf["grad"][i] for i in range(iters)],
            "flow_mono": leaf["flow_mono"], "flow_init": leaf["flow_init"], "cost_volume": leaf["cost_volume"]}


def init_mask(flow, valid, D):
    """init_loss's quarter-resolution mask in PyTorch ops, as torch_objective forms it, on the inputs' device."""
    v = ((valid >= 0.5) & (torch.sum(flow ** 2, dim=1).sqrt() < 700)).unsqueeze(1)
    fs = 0.25 * F.interpolate(flow, scale_factor=0.25, mode="nearest")
    vi = (F.interpolate(v.float(), scale_factor=0.25, mode="bilinear", align_corners=True) == 1) & (fs.abs() < 175)
    idx = torch.arange(fs.size(3), device=fs.device).view(1, 1, 1, -1) + fs
    return (idx >= 0) & (idx <= D - 1) & vi


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, nargs="+", default=[5, 32])
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    assert a.reps >= 20
    from tcs_mi355 import native, synth, train_losses
    native.lib()
    dev = torch.device("cuda:0")
    for B, H, W in ((1, 480, 640), (4, 320, 720)):
        for iters in a.iters:
            c = {k: torch.from_numpy(v).to(dev) for k, v in synth.make_loss_case(1, B, H, W, iters).items()}
            leaf = {k: c[k].clone().requires_grad_(True) for k in LEAVES}
            out = as_output(leaf, iters)

            def clear():
                for t in leaf.values():
                    t.grad = None

            def hip_step():
                clear()
                train_losses.training_objective(out, c["flow"], c["valid"], sync=False)[0].backward()

            def hip_forward():
                train_losses.training_objective(out, c["flow"], c["valid"], sync=False)

            def torch_step():
                clear()
                torch_objective(out, c["flow"], c["valid"])[0].backward()

            def torch_forward():
                torch_objective(out, c["flow"], c["valid"])

            res = {"shape": [B, H, W], "iters": iters, "reps": a.reps,
                   "hip_fwd_bwd_ms": timed(hip_step, a.reps), "hip_fwd_ms": timed(hip_forward, a.reps),
                   "torch_fwd_bwd_ms": timed(torch_step, a.reps), "torch_fwd_ms": timed(torch_forward, a.reps)}
            res["speedup_fwd_bwd"] = round(res["torch_fwd_bwd_ms"] / res["hip_fwd_bwd_ms"], 2)
            # the gradients of the two paths on this shape (signs and masks agree except on kinks)
            hip_step()
            g_hip = {k: t.grad.clone() for k, t in leaf.items()}
            torch_step()
            res["max_abs_diff_over_max_grad"] = {k: float((g_hip[k] - t.grad).abs().max() / t.grad.abs().max()) for k, t in leaf.items()}
            res["elements_off_by_1e-5_of_max"] = {k: int(((g_hip[k] - t.grad).abs() > 1e-5 * t.grad.abs().max()).sum())
                                                  for k, t in leaf.items()}
            # the same PyTorch objective on the CPU, whose mask rules the kernels are pinned to, and how many
            # pixels of init_loss's mask PyTorch's GPU ops decide differently: one such pixel changes the count N_m, hence every entry
            cpu_leaf = {k: c[k].cpu().clone().requires_grad_(True) for k in LEAVES}
            torch_objective(as_output(cpu_leaf, iters), c["flow"].cpu(), c["valid"].cpu())[0].backward()
            res["max_abs_diff_over_max_grad_vs_torch_cpu"] = {k: float((g_hip[k].cpu() - t.grad).abs().max() / t.grad.abs().max())
                                                              for k, t in cpu_leaf.items()}
            # the cost volume by columns: which columns each side masks (a column outside init_loss's mask is all zero), and the
            # difference on the columns both mask once each side is multiplied by its own mask count N_m
            gh, gt = g_hip["cost_volume"].cpu().double(), cpu_leaf["cost_volume"].grad.double()
            ca, cb = (gh != 0).any(1), (gt != 0).any(1)
            both = (ca & cb).unsqueeze(1)
            na, nb = float(ca.sum()), float(cb.sum())
            res["cost_volume_columns"] = {"hip": int(na), "torch_cpu": int(nb), "one_side_only": int((ca != cb).sum()),
                                          "max_abs_diff_both_times_count": float(((gh * na - gt * nb).abs() * both).max())}
            m_gpu, m_cpu = init_mask(c["flow"], c["valid"], W // 4).cpu(), init_mask(c["flow"].cpu(), c["valid"].cpu(), W // 4)
            res["init_mask_pixels_torch_gpu_vs_cpu"] = {"differ": int((m_gpu != m_cpu).sum()), "gpu": int(m_gpu.sum()), "cpu": int(m_cpu.sum())}
            # device time of the backward launches alone
            total = train_losses.training_objective(out, c["flow"], c["valid"], sync=False)[0]
            for _ in range(3):
                clear()
                total.backward(retain_graph=True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.reps):
                clear()
                total.backward(retain_graph=True)
            e1.record()
            torch.cuda.synchronize()
            res["hip_bwd_device_ms"] = round(e0.elapsed_time(e1) / a.reps, 4)
            res["bwd_bytes"] = bytes_needed(B, H, W, iters)
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
