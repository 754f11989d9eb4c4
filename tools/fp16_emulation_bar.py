"""The accuracy bar of the fp16 precision mode (TCStereo hip_precision="fp16"), measured on the CPU oracle.

Runs oracle/tcs_oracle.py twice on the same inputs: once as it is (fp32), once with the operands of exactly the convolutions the mode
covers rounded the way the single-product kernels round them: activations to f16(clamp(x, +-65504)), weights to f16(w * 2^s) * 2^-s with
the packing's per-layer scale s = 12 - floor(log2 max|w|).  Left unrounded, as on the GPU: the 7x7 stems and the single-input-channel
layers (fp32 kernels), the gradient stems' first layers (pinned to fp32 MFMA), the HiddenstateUpdater (fused kernel, fp16-split in both
modes) and the two convolutions folded into their producer as tap partials (flow_head.conv2, residual_head.2).  Prints one JSON line with
the EPE of the rounded run against the plain one at BASELINE config 1 (320x240 padded to 320x256, 8 iterations) and config 2 frame 0
(640x480, 32 iterations).  tests/test_gpu_precision.py derives its end-to-end bar from these numbers.

    python tools/fp16_emulation_bar.py [--configs c1,c2]
"""
import argparse
import contextlib
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tcs_paths  # noqa: E402

tcs_paths.add_product_path()
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import torch  # noqa: E402

# layers the fp16 mode leaves fp16-split or fp32 (core/tc_stereo.py, core/update.py: products_of / _tcs_math)
EXEMPT_PREFIXES = ("hiddenstate_update.", "update_block.flow_head.conv2.", "disp_grad_refine.residual_head.2.",
                   "disp_grad_refine.conv_grad_stem.0.", "disp_grad_refine.conv_grad_candidate_stem.0.")


def round_act(x):
    return x.clamp(-65504.0, 65504.0).half().float()


def round_weight(w):
    wmax = float(w.abs().max())
    s = 0 if wmax == 0.0 else max(-40, min(40, int(12 - math.floor(math.log2(wmax)))))
    return (w * 2.0 ** s).half().float() * 2.0 ** (-s)


class _RoundedF:
    """Stands in for torch.nn.functional inside the oracle module: conv2d / conv_transpose2d round the operands of covered layers."""

    def __init__(self, F, exempt_ids):
        self._F, self._exempt = F, exempt_ids
        self.calls = {"rounded": 0, "kept": 0}

    def __getattr__(self, name):
        return getattr(self._F, name)

    def _covered(self, w, cin):
        return id(w) not in self._exempt and w.shape[-1] in (1, 3, 4) and cin > 1

    def conv2d(self, x, w, b=None, stride=1, padding=0, *a, **kw):
        if self._covered(w, int(w.shape[1])):
            self.calls["rounded"] += 1
            x, w = round_act(x), round_weight(w)
        else:
            self.calls["kept"] += 1
        return self._F.conv2d(x, w, b, stride, padding, *a, **kw)

    def conv_transpose2d(self, x, w, b=None, stride=1, padding=0, *a, **kw):
        if self._covered(w, int(w.shape[0])):
            self.calls["rounded"] += 1
            x, w = round_act(x), round_weight(w)
        else:
            self.calls["kept"] += 1
        return self._F.conv_transpose2d(x, w, b, stride, padding, *a, **kw)


@contextlib.contextmanager
def fp16_operands(oracle, W):
    """Within the block, oracle.tc_stereo_forward(W, ...) computes what the fp16 mode computes (to fp32 summation order)."""
    exempt = {id(v) for k, v in W.items() if k.startswith(EXEMPT_PREFIXES)}
    saved = oracle.F
    oracle.F = _RoundedF(saved, exempt)
    try:
        yield oracle.F
    finally:
        oracle.F = saved


def inputs(config):
    from tcs_mi355 import synth
    from tcs_mi355.harness import InputPadder
    if config == "c1":
        pr = synth.make_pair(1)
        i1, i2 = InputPadder(pr.image1[None].shape, divis_by=32).pad(torch.as_tensor(pr.image1)[None], torch.as_tensor(pr.image2)[None])
        return i1, i2, 8
    fr = synth.make_sequence(2000, n_frames=1).frames[0]
    return torch.as_tensor(fr.image1)[None], torch.as_tensor(fr.image2)[None], 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c1,c2")
    args = ap.parse_args()
    import tcs_oracle as oracle
    from tcs_mi355.weights import synth_state_dict
    with open(os.path.join(ROOT, "tests", "golden", "state_dict_keys.json")) as f:
        W = synth_state_dict(json.load(f)["shared_backbone"])
    torch.set_num_threads(max(1, os.cpu_count() or 1))
    out = {"what": "EPE of the oracle with fp16-rounded operands on the layers the fp16 mode covers, against the plain fp32 oracle"}
    for cfg in args.configs.split(","):
        i1, i2, iters = inputs(cfg)
        t0 = time.time()
        with torch.no_grad():
            ref = oracle.tc_stereo_forward(W, i1.float(), i2.float(), iters=iters)
            with fp16_operands(oracle, W) as rf:
                got = oracle.tc_stereo_forward(W, i1.float(), i2.float(), iters=iters)
        row = {"iters": iters, "shape": list(i1.shape[2:]), "seconds": round(time.time() - t0, 1), "layer_calls": dict(rf.calls)}
        for k in ("flow", "flow_q"):
            if k in ref:
                row[f"epe_{k}"] = float((got[k].double() - ref[k].double()).abs().mean())
        out[cfg] = row
        print(json.dumps({cfg: row}), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
