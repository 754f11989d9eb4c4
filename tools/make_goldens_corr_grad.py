#!/usr/bin/env python3
"""Reference-generated gradients of the correlation block (core/corr.py:7-79): tests/golden/corr_grad.npz.

Runs in the build container only.  It imports the reference's CorrBlock1D (make_goldens.import_reference) and differentiates one
training step's use of it on the CPU in float32 with torch autograd: three lookups (corr.py:33-52, grid_sample), the masked cost
volume (corr.py:64-65) and argmax_disp's main_cost (corr.py:67-79), scored as
  L = sum_k <lookup(coords_k), g_lookup_k> + <cost_volume, g_cost> + <main_cost, g_main>.
The inputs are not stored: the tests regenerate them with synth.make_corr_grad_case and check the digest stored here.
  grad_fmap1, grad_fmap2 [B,C,H,W]   grad_coords [3,B,1,H,W]   digest   case [seed, B, C, H, W, radius]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_goldens as mg  # noqa: E402

CASE = (11, 1, 256, 3, 44, 4)        # seed, B, C, H, W (ragged: not a multiple of 64 or of 8), radius


def digest(case):
    return mg.sha(*[case[key] for key in sorted(case)])


def main():
    torch.set_num_threads(8)
    _, ref_corr, *_ = mg.import_reference()
    synth = mg.load_by_path("tcs_synth", os.path.join(mg.PKG, "tcs_mi355", "synth.py"))
    seed, B, C, H, W, r = CASE
    case = synth.make_corr_grad_case(seed, B, C, H, W, r)
    f1 = torch.from_numpy(case["fmap1"]).requires_grad_(True)
    f2 = torch.from_numpy(case["fmap2"]).requires_grad_(True)
    coords = [torch.from_numpy(c).requires_grad_(True) for c in case["coords"]]
    blk = ref_corr.CorrBlock1D(f1, f2, num_levels=4, radius=r)
    loss = sum((blk(c) * torch.from_numpy(g)).sum() for c, g in zip(coords, case["g_lookup"]))
    loss = loss + (blk.get_cost_volume() * torch.from_numpy(case["g_cost"])).sum()
    loss = loss + (blk.argmax_disp()[1] * torch.from_numpy(case["g_main"])).sum()
    loss.backward()
    res = {"grad_fmap1": f1.grad.numpy(), "grad_fmap2": f2.grad.numpy(),
           "grad_coords": np.stack([c.grad.numpy() for c in coords]), "digest": np.array(digest(case)),
           "case": np.array(CASE, np.int64)}
    out = os.path.join(ROOT, "tests", "golden", "corr_grad.npz")
    np.savez_compressed(out, **res)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
