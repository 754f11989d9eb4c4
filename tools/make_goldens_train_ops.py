#!/usr/bin/env python3
"""Reference-generated values and gradients of the two training ops of tcs_mi355.train_ops: tests/golden/train_ops.npz.

Runs in the build container only, on the CPU in float32.  It imports the reference as tools/make_goldens.py does and runs
  * its own `TCStereo.upsample_flow` twice on one mask, as tc_stereo.py:213-214 do (flow_a with the mask detached, flow_b with it), and
  * its own `DispRefine.forward` with `w_head` replaced by a module that returns the case's logits, so that lines 292-300 run on given
    inputs (the other convolutions still run, on zeros; nothing of them reaches the outputs kept here),
then stores the inputs, the upstream gradients, the outputs and torch.autograd.grad of sum(out * upstream).  Data only.
Per case i (CASES order):
  c{i}_flow_a, c{i}_flow_b [B,1,H,W]   c{i}_mask [B,144,H,W]   c{i}_g_a, c{i}_g_b [B,1,4H,4W] (upstream)
  c{i}_up_a, c{i}_up_b [B,1,4H,4W]     c{i}_dflow_a, c{i}_dflow_b [B,1,H,W]   c{i}_dmask [B,144,H,W]
  c{i}_logits [B,9,H,W]  c{i}_disp_grads [B,2,H,W]  c{i}_disp [B,1,H,W]  c{i}_g_r [B,1,H,W] (upstream)
  c{i}_refined [B,1,H,W]  c{i}_dlogits [B,9,H,W]  c{i}_ddisp_grads [B,2,H,W]
  cases [n, 5]   seed, B, H, W, logit spread (logits uniform in +-spread; 30 saturates the softmax)
"""
import os
import sys
from argparse import Namespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_goldens as mg  # noqa: E402

# ragged sizes, B = 1 and 2, a single row, a single column, and a saturated softmax
CASES = [(11, 1, 5, 7, 3), (12, 2, 6, 11, 3), (13, 1, 1, 9, 3), (14, 1, 8, 1, 3), (15, 2, 5, 7, 30)]


def make_case(seed, B, H, W, spread):
    """The inputs of one case, float32: disparities of tens of pixels (flow = -disp), gradients of a fraction of a pixel per pixel."""
    g = torch.Generator().manual_seed(seed)

    def u(*shape, lo=-1.0, hi=1.0):
        return lo + (hi - lo) * torch.rand(*shape, generator=g)
    return {"flow_a": -u(B, 1, H, W, lo=1, hi=40), "flow_b": -u(B, 1, H, W, lo=1, hi=40), "mask": u(B, 144, H, W) * spread,
            "g_a": torch.randn(B, 1, 4 * H, 4 * W, generator=g), "g_b": torch.randn(B, 1, 4 * H, 4 * W, generator=g),
            "logits": u(B, 9, H, W) * spread, "disp_grads": 0.3 * torch.randn(B, 2, H, W, generator=g),
            "disp": u(B, 1, H, W, lo=1, hi=40), "g_r": torch.randn(B, 1, H, W, generator=g)}


def no_ties(x, dim):
    top = torch.topk(x, 2, dim=dim).values
    return bool((top.select(dim, 0) != top.select(dim, 1)).all())


class Given(torch.nn.Module):
    def __init__(self, value):
        super().__init__()
        self.value = value

    def forward(self, _):
        return self.value


def reference_results(ref_tc, ref_update, c):
    B, _, H, W = c["flow_a"].shape
    assert no_ties(c["mask"].view(B, 9, 16, H, W), 1) and no_ties(c["logits"], 1)
    model = Namespace(args=Namespace(n_downsample=2))
    fa, fb, mask = (c[k].clone().requires_grad_(True) for k in ("flow_a", "flow_b", "mask"))
    up_a = ref_tc.TCStereo.upsample_flow(model, fa, mask.detach())
    up_b = ref_tc.TCStereo.upsample_flow(model, fb, mask)
    dfa, dfb, dm = torch.autograd.grad((up_a * c["g_a"]).sum() + (up_b * c["g_b"]).sum(), [fa, fb, mask])
    refine = ref_update.DispRefine(Namespace(n_downsample=2))
    logits, grads = c["logits"].clone().requires_grad_(True), c["disp_grads"].clone().requires_grad_(True)
    refine.w_head = Given(logits)
    refined, _ = refine(grads, c["disp"], torch.zeros(B, 128, H, W), torch.zeros(B, 64, H, W), test_mode=True)
    dl, dg = torch.autograd.grad((refined * c["g_r"]).sum(), [logits, grads])
    return {"up_a": up_a, "up_b": up_b, "dflow_a": dfa, "dflow_b": dfb, "dmask": dm, "refined": refined, "dlogits": dl, "ddisp_grads": dg}


def main():
    torch.set_num_threads(8)
    ref_tc, _, ref_update, *_ = mg.import_reference()
    out = {"cases": np.array(CASES, np.int64)}
    for i, case in enumerate(CASES):
        c = make_case(*case)
        r = reference_results(ref_tc, ref_update, c)
        for key, v in {**c, **r}.items():
            out[f"c{i}_{key}"] = v.detach().numpy().astype(np.float32)
        print(i, case, {k: float(v.abs().max()) for k, v in r.items()})
    path = os.path.join(ROOT, "tests", "golden", "train_ops.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
