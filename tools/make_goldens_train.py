#!/usr/bin/env python3
"""Reference-generated vectors for TCStereo.forward(test_mode=False), the training-output dict (tc_stereo.py:204-243).

Runs in the build container only, like tools/make_goldens.py, whose reference import (the stub `cupy` module) it reuses.  The
temporal frame goes through the same CPU stand-in for `softsplat_func.apply` (the oracle's `softsplat_forward`), so its vectors are
restatement-pinned for the splat and reference arithmetic for everything else.  Weights: the key-seeded damped synthetic ones.

One 128x160 sequence (32x40 feature grid): a first frame and one temporal frame, 4 iterations each, every key of the dict.  The
low-resolution maps are stored whole; the full-resolution maps and the cost volume at a fixed seeded sample of their elements (the
index arrays are in the file), and net_list / fmap1 — which test mode returns too, pinned by tests/golden/e2e.npz — as per-channel sums,
so that the file stays a few hundred KiB.  Per frame t (0, 1), the per-iteration lists stacked:
  f{t}_flow_predictions        [iters, 2, NS_UP]   ([flows_up, flow_refine_up] per iteration, flattened [1,1,128,160] at `idx_up`)
  f{t}_flow_q_predictions      [iters, 2, 1, 1, 32, 40]     ([-disp_q, -refined_disp])
  f{t}_disp_grad_q_predictions [iters, 1, 2, 32, 40]
  f{t}_flow_mono, f{t}_flow_init [NS_UP] (at `idx_up`); f{t}_cost_volume [NS_CV] (flattened [1,40,32,40] at `idx_cv`)
  f{t}_flow_q [1, 1, 32, 40]; f{t}_net{i}_sum [1, 128] and f{t}_fmap1_sum [1, 256] (sums over H, W)
plus `input_sha` (the images, as the other goldens record them).  Writes tests/golden/train_outputs.npz.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_goldens as mg  # noqa: E402

SEQ = dict(seed=7, n_frames=2, height=128, width=160, max_disp=48.0)
ITERS = 4
NS_UP, NS_CV = 2048, 4096           # sampled elements of a full-resolution map (of 20480) and of the cost volume (of 51200)


def sample_indices(n, k, seed):
    """Sorted, distinct flat indices: k of range(n), drawn from `seed` only."""
    g = np.random.Generator(np.random.Philox(key=seed))
    return np.sort(g.choice(n, size=k, replace=False)).astype(np.int32)


def main():
    torch.set_num_threads(8)
    ref_tc, ref_corr, ref_update, ref_geo, ref_utils, ref_splat = mg.import_reference()
    weights = mg.load_by_path("tcs_weights", os.path.join(mg.PKG, "tcs_mi355", "weights.py"))
    synth = mg.load_by_path("tcs_synth", os.path.join(mg.PKG, "tcs_mi355", "synth.py"))
    oracle = mg.load_by_path("tcs_oracle", os.path.join(ROOT, "oracle", "tcs_oracle.py"))

    class _Splat:
        @staticmethod
        def apply(tin, tflow):
            return oracle.softsplat_forward(tin, tflow)
    ref_splat.softsplat_func = _Splat

    from argparse import Namespace
    args = Namespace(hidden_dims=[128] * 3, shared_backbone=True, corr_levels=4, corr_radius=4, n_downsample=2, context_norm="none",
                     slow_fast_gru=False, n_gru_layers=3, mixed_precision=False, init_thres=0.5)
    model = ref_tc.TCStereo(args).eval()
    weights.load_synth_weights(model)

    seq = synth.make_sequence(SEQ["seed"], n_frames=SEQ["n_frames"], height=SEQ["height"], width=SEQ["width"], max_disp=SEQ["max_disp"])
    res = {"input_sha": np.frombuffer(mg.sha(*[f.image1 for f in seq.frames], *[f.image2 for f in seq.frames]).encode(), dtype=np.uint8),
           "iters": np.array(ITERS, np.int32),
           "idx_up": sample_indices(SEQ["height"] * SEQ["width"], NS_UP, 41),
           "idx_cv": sample_indices((SEQ["width"] // 4) * (SEQ["height"] // 4) * (SEQ["width"] // 4), NS_CV, 42)}
    up = lambda x: mg.N(x).reshape(-1)[res["idx_up"]]
    K = mg.T(seq.K)[None]
    bl = torch.tensor([seq.baseline])
    params, flow_q, fmap1, prev_T, nets = {}, None, None, None, None
    with torch.no_grad():
        for t, fr in enumerate(seq.frames):
            Tt = mg.T(fr.T)[None]
            params.update(K=K, T=Tt, previous_T=prev_T, last_disp=flow_q, last_net_list=nets, fmap1=fmap1, baseline=bl)
            o = model(mg.T(fr.image1)[None], mg.T(fr.image2)[None], iters=ITERS, test_mode=False,
                      params=params if flow_q is not None else None)
            flow_q, nets, fmap1, prev_T = o["flow_q"], o["net_list"], o["fmap1"], Tt
            p = f"f{t}_"
            res[p + "flow_predictions"] = np.stack([np.stack([up(a), up(b)]) for a, b in o["flow_predictions"]])
            res[p + "flow_q_predictions"] = np.stack([np.stack([mg.N(a), mg.N(b)]) for a, b in o["flow_q_predictions"]])
            res[p + "disp_grad_q_predictions"] = np.stack([mg.N(g) for g in o["disp_grad_q_predictions"]])
            res[p + "flow_mono"], res[p + "flow_init"] = up(o["flow_mono"]), up(o["flow_init"])
            res[p + "cost_volume"] = mg.N(o["cost_volume"]).reshape(-1)[res["idx_cv"]]
            res[p + "flow_q"] = mg.N(o["flow_q"])
            for i, n in enumerate(o["net_list"]):
                res[p + f"net{i}_sum"] = mg.N(n.sum((2, 3)))
            res[p + "fmap1_sum"] = mg.N(o["fmap1"].sum((2, 3)))
            print("frame", t, "|flow_refine_up| mean per iteration",
                  [round(float(b.abs().mean()), 4) for _, b in o["flow_predictions"]], "GT", float(fr.disp_gt.mean()))
    path = os.path.join(mg.OUT, "train_outputs.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
