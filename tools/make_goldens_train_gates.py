#!/usr/bin/env python3
"""Reference-generated values and gradients of the recurrent cells' gate arithmetic (tcs_mi355.train_ops.gru_reset / gru_update):
tests/golden/train_gates.npz.

Runs in the build container only, on the CPU in float32.  It imports the reference as tools/make_goldens_train_ops.py does and runs
its own `ConvGRU.forward`, `Lightfuse.forward` and `HiddenstateUpdater.forward` with the convolutions replaced by stand-ins, so that
the gate lines (update.py:81-85, 30-34, 62-66) run on given inputs:
  * `convzr` returns a leaf zr [B,2C,H,W] (chunked by the reference into the pre-activations of z and r),
  * `convq` returns x[:, :C] * wq + q0 with wq, q0 leaves: r*h reaches the output through a known factor, q0 plays q_pre,
  * `HiddenstateUpdater.convs` returns a given tensor.
Stores the inputs, the upstream gradient, h_new and torch.autograd.grad of sum(h_new * upstream).  Data only.
Per cell (gru = ConvGRU, fuse = Lightfuse, hu = HiddenstateUpdater) and case i (CASES order), all [B,C,H,W] but zr [B,2C,H,W]:
  {cell}_c{i}_zr, _q0, _wq, _h, _g (upstream)        gru only: _cz, _cr, _cq
  {cell}_c{i}_h_new, _dzr, _dq0, _dh                 gru only: _dcz, _dcr, _dcq
  cases [n, 6]   seed, B, C, H, W, spread (pre-activations are spread * randn; 30 saturates the gates); h is uniform in (-1, 1)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_goldens as mg  # noqa: E402

# ragged planes (H*W = 35), a batch whose stride matters, a single element, H*W a multiple of 4, and saturated gates
CASES = [(21, 1, 3, 5, 7, 2), (22, 2, 5, 6, 11, 2), (23, 1, 1, 1, 1, 2), (24, 1, 4, 4, 8, 2), (25, 2, 3, 5, 7, 30)]
CELLS = ("gru", "fuse", "hu")


def make_case(seed, B, C, H, W, spread, cell):
    g = torch.Generator().manual_seed(seed * 10 + CELLS.index(cell))

    def n(*shape):
        return torch.randn(*shape, generator=g)
    c = {"zr": spread * n(B, 2 * C, H, W), "q0": spread * n(B, C, H, W), "wq": n(B, C, H, W),
         "h": 2 * torch.rand(B, C, H, W, generator=g) - 1, "g": n(B, C, H, W)}
    if cell == "gru":
        c.update(cz=n(B, C, H, W), cr=n(B, C, H, W), cq=n(B, C, H, W))
    return c


class Given(torch.nn.Module):
    def __init__(self, value):
        super().__init__()
        self.value = value

    def forward(self, _):
        return self.value


class ScaledHead(torch.nn.Module):
    """x[:, :C] * wq + q0: the stand-in for convq (x = cat(r * h, ...))."""

    def __init__(self, wq, q0):
        super().__init__()
        self.wq, self.q0 = wq, q0

    def forward(self, x):
        return x[:, :self.wq.shape[1]] * self.wq + self.q0


def reference_results(ref_update, cell, c):
    B, C, H, W = c["h"].shape
    L = {k: v.clone().requires_grad_(True) for k, v in c.items() if k not in ("g", "wq")}
    if cell == "gru":
        m = ref_update.ConvGRU(C, 2)
    elif cell == "fuse":
        m = ref_update.Lightfuse(C, 2)
    else:
        m = ref_update.HiddenstateUpdater(C)
        m.convs = Given(torch.zeros(B, 64, H, W))
    m.convzr, m.convq = Given(L["zr"]), ScaledHead(c["wq"], L["q0"])
    if cell == "gru":
        h_new = m(L["h"], L["cz"], L["cr"], L["cq"], torch.zeros(B, 2, H, W))
    else:
        h_new = m(L["h"], torch.zeros(B, 1 if cell == "hu" else 2, H, W))
    names = ["zr", "q0", "h"] + (["cz", "cr", "cq"] if cell == "gru" else [])
    grads = torch.autograd.grad((h_new * c["g"]).sum(), [L[k] for k in names])
    return {"h_new": h_new, **{"d" + k: v for k, v in zip(names, grads)}}


def main():
    torch.set_num_threads(8)
    _, _, ref_update, *_ = mg.import_reference()
    out = {"cases": np.array(CASES, np.int64)}
    for cell in CELLS:
        for i, case in enumerate(CASES):
            c = make_case(*case, cell)
            r = reference_results(ref_update, cell, c)
            for key, v in {**c, **r}.items():
                out[f"{cell}_c{i}_{key}"] = v.detach().numpy().astype(np.float32)
            print(cell, i, case, {k: float(v.abs().max()) for k, v in r.items()})
    path = os.path.join(ROOT, "tests", "golden", "train_gates.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
