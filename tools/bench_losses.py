#!/usr/bin/env python3
"""Time per frame of the training objective (train_stereo.py:362-399) at 640x480: tcs_mi355.losses.training_objective (five HIP
launches, one host synchronisation) against the same objective restated in PyTorch on the GPU the way the trainer runs it (its
ATen ops and a .item() per metric).  Prints one JSON line per iteration count.

    python tools/bench_losses.py [--iters 5 32] [--reps 50]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tcs_paths  # noqa: E402

tcs_paths.add_product_path()
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def _median_pool4(x):
    u = x.unfold(2, 4, 4).unfold(3, 4, 4)
    return u.contiguous().view(u.size()[:4] + (-1,)).median(dim=-1)[0]


def _grad(d):
    p = F.pad(d, (1, 1, 1, 1), mode="replicate")
    return torch.cat((p[:, :, 1:-1, 2:] - p[:, :, 1:-1, 1:-1], p[:, :, 2:, 1:-1] - p[:, :, 1:-1, 1:-1]), 1)


def _normal(d):
    g = _grad(d)
    return F.normalize(torch.cat((g, -torch.ones_like(g[:, :1])), 1), dim=1)


def torch_objective(out, flow, valid, k=3, thr=0.5):
    """The reference's four losses in PyTorch (fp32, on the inputs' device), metrics read with .item() as the trainer does."""
    n = len(out["flow_predictions"])
    g = 0.9 ** (15 / (n - 1))
    w = [g ** (n - i - 1) for i in range(n)]
    m = {}
    mag = torch.sum(flow ** 2, dim=1).sqrt()
    v = ((valid >= 0.5) & (mag < 700)).unsqueeze(1)
    gg = _grad(-flow)
    ng = F.normalize(torch.cat((gg, -torch.ones_like(gg[:, :1])), 1), dim=1)
    # sequence_loss
    seq = 0.1 * (out["flow_init"] - flow).abs()[v].mean() + 0.1 * (out["flow_mono"] - flow).abs()[v].mean()
    for i, (a, b) in enumerate(out["flow_predictions"]):
        assert not torch.isnan(a).any() and not torch.isinf(a).any()
        seq = seq + w[i] * ((a - flow).abs() + 1.2 * (b - flow).abs())[v].mean()
    epe = torch.sum((out["flow_predictions"][-1][0] - flow) ** 2, dim=1).sqrt().view(-1)[v.view(-1)]
    epr = torch.sum((out["flow_predictions"][-1][1] - flow) ** 2, dim=1).sqrt().view(-1)[v.view(-1)]
    epi = torch.sum((out["flow_init"] - flow) ** 2, dim=1).sqrt().view(-1)[v.view(-1)]
    m.update(epe=epe.mean().item(), epe_refine=epr.mean().item(), epe_init=epi.mean().item())
    for t in (1, 3, 5):
        m[f"{t}px"] = (epe < t).float().mean().item()
        m[f"{t}px_refine"] = (epr < t).float().mean().item()
    # init_loss
    cv = out["cost_volume"]
    D = cv.size(1)
    fs = 0.25 * F.interpolate(flow, scale_factor=0.25, mode="nearest")
    vi = (F.interpolate(v.float(), scale_factor=0.25, mode="bilinear", align_corners=True) == 1) & (fs.abs() < 175)
    idx = torch.arange(cv.size(3), device=cv.device).view(1, 1, 1, -1) + fs
    mask = (idx >= 0) & (idx <= D - 1) & vi
    idx = idx.clamp(0, D - 1)
    df = idx.floor().long()
    fr = idx - df
    phi = fr * cv.gather(1, (df + 1).clamp(0, D - 1)) + (1 - fr) * cv.gather(1, df)
    gl = 1 - phi[mask].mean()
    cand = torch.arange(D, device=cv.device).view(1, -1, 1, 1)
    excl = ((cand >= idx - 1.5) & (cand < idx + 1.5)) | ~mask
    top = torch.topk(cv.masked_fill(excl, 0), k=k, dim=1).values
    nml = (top + thr - phi.detach()).clamp(min=0)[mask.repeat(1, k, 1, 1)].mean()     # train_stereo.py:171 (same value; matters under backward)
    ini = gl + nml
    m.update(init_loss=ini.item(), init_gt_loss=gl.item(), init_nm_loss=nml.item(),
             forward_mask_rate=((top[:, :1] + 0.3 - phi) > 0).float().mean().item())
    # disp_normal_loss / disp_grad_loss
    qv = F.max_pool2d(v.float(), 4, 4, 0).bool()
    gp, npool = _median_pool4(gg), _median_pool4(ng)
    gv = qv & (gp[:, :1] < 5) & (gp[:, 1:] < 5)
    nv = qv & (npool[:, :1] / npool[:, 2:] < 5) & (npool[:, 1:2] / npool[:, 2:] < 5)
    norm = 0.0
    for i, (a, b) in enumerate(out["flow_q_predictions"]):
        la = 0.5 * (_normal(-a) - npool).abs().mean(1, keepdim=True) + 0.5 * (1 - (_normal(-a) * npool).sum(1, keepdim=True))
        lb = 0.5 * (_normal(-b) - npool).abs().mean(1, keepdim=True) + 0.5 * (1 - (_normal(-b) * npool).sum(1, keepdim=True))
        norm = norm + w[i] * (la[nv].mean() + 1.2 * lb[nv].mean())
    grad = 0.0
    for i, p in enumerate(out["disp_grad_q_predictions"]):
        assert not torch.isnan(p).any() and not torch.isinf(p).any()
        grad = grad + w[i] * (p - gp).abs().mean(1, keepdim=True)[gv].mean()
    m.update(norm_loss=norm.item(), grad_loss=grad.item())
    return seq + ini + 0.25 * norm + 5 * grad, m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, nargs="+", default=[5, 32])
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    from tcs_mi355 import losses, native, synth
    native.lib()
    dev = torch.device("cuda:0")
    for iters in a.iters:
        c = {k: torch.from_numpy(v).to(dev) for k, v in synth.make_loss_case(1, 1, 480, 640, iters).items()}
        out = {"flow_predictions": [[c["up"][i, 0], c["up"][i, 1]] for i in range(iters)],
               "flow_q_predictions": [[c["q"][i, 0], c["q"][i, 1]] for i in range(iters)],
               "disp_grad_q_predictions": [c["grad"][i] for i in range(iters)],
               "flow_mono": c["flow_mono"], "flow_init": c["flow_init"], "cost_volume": c["cost_volume"]}
        res = {"iters": iters, "shape": [480, 640]}
        for name, fn in (("hip", lambda: losses.training_objective(out, c["flow"], c["valid"])),
                         ("torch", lambda: torch_objective(out, c["flow"], c["valid"]))):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                _, met = fn()
            torch.cuda.synchronize()
            res[f"{name}_ms_per_frame"] = round((time.perf_counter() - t0) * 1e3 / a.reps, 4)
            res[f"{name}_total_and_epe"] = [met["grad_loss"], met["epe"]]
        # device time of the five launches alone (no host synchronisation inside the window)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            losses.training_objective(out, c["flow"], c["valid"], sync=False)
        e1.record()
        torch.cuda.synchronize()
        res["hip_nosync_ms_per_frame"] = round(e0.elapsed_time(e1) / a.reps, 4)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
