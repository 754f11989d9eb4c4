#!/usr/bin/env python3
"""Reference-generated vectors for the training objective (train_stereo.py:41-180, 362-399): tests/golden/losses.npz.

Runs in the build container only.  It imports the reference's train_stereo.py with stand-ins for what the loss functions never
touch (`wandb`, `core.stereo_datasets`, `evaluate_stereo`; `cupy` as tools/make_goldens.py stubs it) and scores the cases of
synth.make_loss_case exactly as the training loop does (lines 362-399), on the CPU in float32.  The inputs are not stored: the tests
regenerate them from the seed and check the digest stored here.  Per case i (CASES order):
  c{i}_seq   [10]  sequence_loss: loss, then SEQ_KEYS (epe, epe_refine, epe_init, 1px, 3px, 5px, 1px_refine, 3px_refine, 5px_refine)
  c{i}_init  [5]   init_loss: loss, then init_loss, init_gt_loss, init_nm_loss, forward_mask_rate
  c{i}_norm, c{i}_grad [2]   disp_normal_loss / disp_grad_loss: loss, metric
  c{i}_total [1]   seq + init + 0.25 norm + 5 grad
  c{i}_digest      sha256 prefix of the inputs (make_goldens.sha over the arrays in sorted key order)
  cases [n, 8]     seed, B, H, W, iters, k, dense_gt, empty
"""
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_goldens as mg  # noqa: E402

# seed, B, H, W, iters, k, dense_gt, empty
CASES = [(1, 1, 32, 48, 3, 3, 1, 0), (2, 2, 32, 40, 4, 1, 0, 0), (3, 2, 36, 44, 2, 3, 1, 0), (4, 1, 32, 48, 3, 3, 0, 1)]


def import_train_stereo():
    mg.import_reference()
    for name in ("wandb", "core.stereo_datasets", "evaluate_stereo"):
        m = types.ModuleType(name)
        m.count_parameters = m.validate_tartanair = m.validate_temporal_things = lambda *a, **k: None
        sys.modules[name] = m
    import train_stereo  # noqa
    return train_stereo


def score(ts, case, c):
    """train_stereo.py:362-399 on one case, the reference's own calls."""
    seed, B, H, W, iters, k, dense, empty = c
    t = {key: torch.from_numpy(v) for key, v in case.items()}
    out = {"flow_predictions": [[t["up"][i, 0], t["up"][i, 1]] for i in range(iters)],
           "flow_q_predictions": [[t["q"][i, 0], t["q"][i, 1]] for i in range(iters)],
           "disp_grad_q_predictions": [t["grad"][i] for i in range(iters)],
           "flow_mono": t["flow_mono"], "flow_init": t["flow_init"], "cost_volume": t["cost_volume"]}
    flow, valid = t["flow"], t["valid"]
    loss_gamma = 0.9
    n = len(out["flow_predictions"])
    g = loss_gamma ** (15 / (n - 1))
    weights = [g ** (n - i - 1) for i in range(n)]
    mag = torch.sum(flow ** 2, dim=1).sqrt()
    valid = ((valid >= 0.5) & (mag < 700)).unsqueeze(1)
    disp_grad_gt, _ = ts.disp2disp_gradient_xy(-flow)
    disp_norm_gt = torch.nn.functional.normalize(torch.cat((disp_grad_gt, -torch.ones_like(disp_grad_gt[:, :1])), dim=1), dim=1)
    seq, seq_m = ts.sequence_loss(out["flow_mono"], out["flow_init"], out["flow_predictions"], flow, valid, weights)
    ini, ini_m = ts.init_loss(out["cost_volume"], flow, valid, k=k, scale=0.25, threshold=0.5)
    nrm, nrm_m = ts.disp_normal_loss(out["flow_q_predictions"], disp_norm_gt, valid, weights, scale=0.25, dense_gt=bool(dense))
    grd, grd_m = ts.disp_grad_loss(out["disp_grad_q_predictions"], disp_grad_gt, valid, weights, scale=0.25, dense_gt=bool(dense))
    seq_keys = ("epe", "epe_refine", "epe_init", "1px", "3px", "5px", "1px_refine", "3px_refine", "5px_refine")
    init_keys = ("init_loss", "init_gt_loss", "init_nm_loss", "forward_mask_rate")
    return {"seq": [float(seq)] + [seq_m[key] for key in seq_keys], "init": [float(ini)] + [ini_m[key] for key in init_keys],
            "norm": [float(nrm), nrm_m["norm_loss"]], "grad": [float(grd), grd_m["grad_loss"]],
            "total": [float(seq + ini + 0.25 * nrm + 5 * grd)]}


def digest(case):
    return mg.sha(*[case[key] for key in sorted(case)])


def main():
    torch.set_num_threads(8)
    ts = import_train_stereo()
    synth = mg.load_by_path("tcs_synth", os.path.join(mg.PKG, "tcs_mi355", "synth.py"))
    res = {"cases": np.array(CASES, np.int64)}
    for i, c in enumerate(CASES):
        seed, B, H, W, iters, k, dense, empty = c
        case = synth.make_loss_case(seed, B, H, W, iters, empty=bool(empty))
        r = score(ts, case, c)
        for key, v in r.items():
            res[f"c{i}_{key}"] = np.array(v, np.float64)
        res[f"c{i}_digest"] = np.array(digest(case))
        print(i, c, {key: np.round(v, 5).tolist() for key, v in r.items()})
    path = os.path.join(ROOT, "tests", "golden", "losses.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
