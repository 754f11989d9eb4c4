#!/usr/bin/env python3
"""Reference-generated gradients of the training objective (train_stereo.py:41-180, 362-399): tests/golden/loss_grad.npz.

Runs in the build container only.  It imports the reference's train_stereo.py as tools/make_goldens_losses.py does, makes the six
predictions of synth.make_loss_case leaves (the stacked `up`, `q`, `grad`, and `flow_mono`, `flow_init`, `cost_volume`), scores lines
362-399 with the reference's own functions on the CPU in float32, and stores torch.autograd.grad of the total and of each part
alone.  Results only; the inputs are regenerated from the seed by the tests and checked against the digest stored here.
Per case i (CASES order):
  c{i}_total_{name}   d total / d name for the six inputs (total = seq + init + 0.25 norm + 5 grad)
  c{i}_seq_{up,flow_mono,flow_init}, c{i}_init_cost_volume, c{i}_norm_q, c{i}_grad_grad   each part alone, w.r.t. what it reads
                      (the four small cases; the large one stores the total's only, to keep the file small)
  c{i}_loss [5]       total, seq, init, norm, grad (NaN on the empty case)
  c{i}_digest         sha256 prefix of the inputs (tools/make_goldens_losses.digest)
  cases [n, 8]        seed, B, H, W, iters, k, dense_gt, empty
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import make_goldens as mg  # noqa: E402
import make_goldens_losses as mgl  # noqa: E402

# the four cases of losses.npz and a larger one (B = 2, 5 iterations)
CASES = mgl.CASES + [(5, 2, 64, 96, 5, 3, 1, 0)]
INPUTS = ("up", "q", "grad", "flow_mono", "flow_init", "cost_volume")
PART_INPUTS = {"seq": ("up", "flow_mono", "flow_init"), "init": ("cost_volume",), "norm": ("q",), "grad": ("grad",)}


def gradients(ts, case, c, parts=True):
    seed, B, H, W, iters, k, dense, empty = c
    t = {key: torch.from_numpy(v) for key, v in case.items()}
    leaf = {n: t[n].clone().requires_grad_(True) for n in INPUTS}
    preds = [[leaf["up"][i, 0], leaf["up"][i, 1]] for i in range(iters)]
    q_preds = [[leaf["q"][i, 0], leaf["q"][i, 1]] for i in range(iters)]
    grad_preds = [leaf["grad"][i] for i in range(iters)]
    flow, valid = t["flow"], t["valid"]
    g = 0.9 ** (15 / (iters - 1))
    weights = [g ** (iters - i - 1) for i in range(iters)]
    mag = torch.sum(flow ** 2, dim=1).sqrt()
    valid = ((valid >= 0.5) & (mag < 700)).unsqueeze(1)
    disp_grad_gt, _ = ts.disp2disp_gradient_xy(-flow)
    disp_norm_gt = F.normalize(torch.cat((disp_grad_gt, -torch.ones_like(disp_grad_gt[:, :1])), dim=1), dim=1)
    seq, _ = ts.sequence_loss(leaf["flow_mono"], leaf["flow_init"], preds, flow, valid, weights)
    ini, _ = ts.init_loss(leaf["cost_volume"], flow, valid, k=k, scale=0.25, threshold=0.5)
    nrm, _ = ts.disp_normal_loss(q_preds, disp_norm_gt, valid, weights, scale=0.25, dense_gt=bool(dense))
    grd, _ = ts.disp_grad_loss(grad_preds, disp_grad_gt, valid, weights, scale=0.25, dense_gt=bool(dense))
    total = seq + ini + 0.25 * nrm + 5 * grd
    res = {"loss": np.array([float(total), float(seq), float(ini), float(nrm), float(grd)], np.float64)}
    alone = [(p, l, PART_INPUTS[p]) for p, l in (("seq", seq), ("init", ini), ("norm", nrm), ("grad", grd))] if parts else []
    for name, loss, wrt in [("total", total, INPUTS)] + alone:
        gs = torch.autograd.grad(loss, [leaf[n] for n in wrt], retain_graph=True, allow_unused=True)
        for n, x in zip(wrt, gs):
            res[f"{name}_{n}"] = (x if x is not None else torch.zeros_like(leaf[n])).numpy().astype(np.float32)
    return res


def main():
    torch.set_num_threads(8)
    ts = mgl.import_train_stereo()
    synth = mg.load_by_path("tcs_synth", os.path.join(mg.PKG, "tcs_mi355", "synth.py"))
    out = {"cases": np.array(CASES, np.int64)}
    for i, c in enumerate(CASES):
        case = synth.make_loss_case(c[0], c[1], c[2], c[3], c[4], empty=bool(c[7]))
        r = gradients(ts, case, c, parts=i < len(mgl.CASES))
        for key, v in r.items():
            out[f"c{i}_{key}"] = v
        out[f"c{i}_digest"] = np.array(mgl.digest(case))
        print(i, c, r["loss"].round(5).tolist(), {k: float(np.abs(v).max()) for k, v in r.items() if k.startswith("total_")})
    path = os.path.join(ROOT, "tests", "golden", "loss_grad.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
