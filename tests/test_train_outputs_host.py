"""TCStereo.forward(test_mode=False) without a GPU: the new C ABI entries, the grad-mode contract, the oracle's restatement of the
reference's non-test branch against tests/golden/train_outputs.npz (tools/make_goldens_train.py), and run_sequence(per_iteration=True)."""
import os
import re
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, ROOT, T

NEW_SYMBOLS = ("tcs_convex_upsample_pair", "tcs_resize_bilinear_scaled")


def _args(**kw):
    d = dict(hidden_dims=[128] * 3, shared_backbone=True, corr_levels=4, corr_radius=4, n_downsample=2,
             context_norm="none", slow_fast_gru=False, n_gru_layers=3, mixed_precision=False, init_thres=0.5)
    d.update(kw)
    return Namespace(**d)


def test_new_entry_points_declared_and_exported():
    from tcs_mi355 import build, native
    build.build(verbose=False)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tcs_mi355.h")).read(), flags=re.S)
    lib = native.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in native.SIGNATURES
        assert hasattr(lib, name)
    assert lib.tcs_abi_version() >= 12


def test_wrappers_validate_before_launching():
    from tcs_mi355 import ops
    d = torch.zeros(1, 1, 4, 6)
    with pytest.raises(ValueError, match="144"):
        ops.convex_upsample_pair(d, d, torch.zeros(1, 9, 4, 6))
    with pytest.raises(ValueError, match="disp_b"):
        ops.convex_upsample_pair(d, torch.zeros(1, 1, 4, 5), torch.zeros(1, 144, 4, 6))
    with pytest.raises(ValueError, match="up_a"):
        ops.convex_upsample_pair(d, d, torch.zeros(1, 144, 4, 6), up_a=torch.zeros(1, 1, 8, 12))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.convex_upsample_pair(d, d, torch.zeros(1, 144, 4, 6))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.resize_bilinear(d, 16, 24, scale=-4.0)


def test_grad_mode_contract():
    from core.tc_stereo import TCStereo
    m = TCStereo(_args()).eval()
    x = torch.zeros(1, 3, 64, 64)
    # grad mode on and trainable parameters: there is no autograd graph to give
    with pytest.raises(NotImplementedError, match="no_grad"):
        m(x, x, iters=1, test_mode=False)
    # under no_grad / inference_mode, or with every parameter frozen, the call gets past that check: CPU tensors are then refused
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU"):
        m(x, x, iters=1, test_mode=False)
    with torch.inference_mode(), pytest.raises(RuntimeError, match="no CPU"):
        m(x, x, iters=1, test_mode=False)
    for p in m.parameters():
        p.requires_grad_(False)
    with pytest.raises(RuntimeError, match="no CPU"):
        m(x, x, iters=1, test_mode=False)
    assert torch.is_grad_enabled()                     # forward does not leak its no_grad
    with pytest.raises(RuntimeError, match="no CPU"):  # test mode: exactly as before
        m(x, x, iters=1, test_mode=True)


def _coords0(fmap):
    n, _, h, w = fmap.shape
    return torch.arange(w, dtype=fmap.dtype).view(1, 1, 1, w).expand(n, 1, h, w).contiguous()


def train_forward(oracle, W, image1, image2, iters, params=None):
    """The reference's non-test branch (tc_stereo.py:96-243, test_mode=False) from the oracle's public functions: the frame's head
    from `tc_stereo_forward`'s trace, the loop restated with want_mask=True on every iteration."""
    args = oracle.default_args()
    tr = {}
    oracle.tc_stereo_forward(W, image1, image2, iters=iters, params=params, args=args, trace=tr)
    fmap1, pyr, inp, grad_ctx = tr["fmap1"], tr["pyr"], tr["inp"], tr["grad_ctx"]
    # disp_mono: the completor again, on the context network's hidden states (the trace keeps the fused ones)
    cnet_list, _ = oracle.context_encoder(W, torch.cat([2 * (image1 / 255.0) - 1.0, 2 * (image2 / 255.0) - 1.0], 0), args.context_norm)
    disp_init, disp_mono, _, _ = oracle.disparity_completor(W, tr["sparse_disp"], tr["cost"], tr["sparse_mask"], [x[0] for x in cnet_list])
    assert torch.allclose(disp_init, tr["disp_init"], atol=1e-5)
    net = [t.clone() for t in tr["net0"]]
    coords0 = _coords0(fmap1)
    coords1 = coords0 - disp_init
    flow_predictions, flow_q_predictions, grads = [], [], []
    for _ in range(iters):
        corr = oracle.corr_lookup(pyr, coords1, args.corr_radius)
        net, delta = oracle.update_block(W, net, inp, corr, coords1 - coords0)
        coords1 = coords1 + delta
        disp_q = coords0 - coords1
        g, gctx = oracle.disp_grad_predictor(W, oracle.disp_gradient_xy(disp_q), disp_q, grad_ctx)
        refined, up_mask = oracle.disp_refine(W, g, disp_q, net[0], gctx, want_mask=True)
        net = [oracle.hidden_state_update(W, net[0], refined - disp_q), net[1], net[2]]
        coords1 = coords0 - refined
        flow_predictions.append([oracle.convex_upsample(-disp_q, up_mask), oracle.convex_upsample(-refined, up_mask)])
        flow_q_predictions.append([-disp_q, -refined])
        grads.append(g)
    up4 = lambda x: -4 * F.interpolate(x, scale_factor=4, mode="bilinear", align_corners=True)
    return {"flow_mono": up4(disp_mono), "flow_init": up4(disp_init), "flow_predictions": flow_predictions,
            "flow_q_predictions": flow_q_predictions, "disp_grad_q_predictions": grads,
            "cost_volume": oracle.masked_cost_volume(oracle.corr_volume(fmap1, tr["fmap2"])),
            "flow_q": (-refined).clamp(max=0), "net_list": net, "fmap1": fmap1}


def as_golden(out, g):
    """A training-output dict in the golden's layout (tools/make_goldens_train.py): per-iteration lists stacked, full-resolution maps and
    the cost volume at the golden's sampled flat indices, net_list / fmap1 as sums over H, W."""
    up = lambda x: x.detach().cpu().reshape(-1)[torch.from_numpy(g["idx_up"]).long()]
    r = {"flow_predictions": torch.stack([torch.stack([up(a), up(b)]) for a, b in out["flow_predictions"]]),
         "flow_q_predictions": torch.stack([torch.stack(p) for p in out["flow_q_predictions"]]).cpu(),
         "disp_grad_q_predictions": torch.stack(out["disp_grad_q_predictions"]).cpu(),
         "flow_mono": up(out["flow_mono"]), "flow_init": up(out["flow_init"]),
         "cost_volume": out["cost_volume"].detach().cpu().reshape(-1)[torch.from_numpy(g["idx_cv"]).long()],
         "flow_q": out["flow_q"].cpu(), "fmap1_sum": out["fmap1"].sum((2, 3)).cpu()}
    r.update({f"net{i}_sum": n.sum((2, 3)).cpu() for i, n in enumerate(out["net_list"])})
    return r


def golden_sequence():
    from tcs_mi355 import synth
    g = dict(np.load(os.path.join(GOLDEN, "train_outputs.npz")))
    seq = synth.make_sequence(7, n_frames=2, height=128, width=160, max_disp=48.0)
    import hashlib
    h = hashlib.sha256()
    for a in [f.image1 for f in seq.frames] + [f.image2 for f in seq.frames]:
        h.update(np.ascontiguousarray(a).tobytes())
    assert h.hexdigest()[:16] == bytes(g["input_sha"]).decode()
    return g, seq


def test_oracle_restatement_matches_reference_golden(oracle, synth_weights):
    g, seq = golden_sequence()
    iters = int(g["iters"])
    K, bl = T(seq.K)[None], torch.tensor([seq.baseline])
    params, flow_q, nets, fmap1, prev_T = {}, None, None, None, None
    for t, fr in enumerate(seq.frames):
        Tt = T(fr.T)[None]
        params.update(K=K, T=Tt, previous_T=prev_T, last_disp=flow_q, last_net_list=nets, fmap1=fmap1, baseline=bl)
        with torch.no_grad():
            out = train_forward(oracle, synth_weights, T(fr.image1)[None], T(fr.image2)[None], iters,
                                params if flow_q is not None else None)
        flow_q, nets, fmap1, prev_T = out["flow_q"], out["net_list"], out["fmap1"], Tt
        p = f"f{t}_"
        for k, v in as_golden(out, g).items():
            assert tuple(v.shape) == g[p + k].shape, k
            if k.endswith("_sum"):         # sums over 1280 .. 5120 elements of O(1) values
                assert float((v - T(g[p + k])).abs().max()) <= 1e-3, (t, k)
            else:
                assert float((v - T(g[p + k])).abs().mean()) <= 1e-5, (t, k)


def test_run_sequence_per_iteration_with_fake_forward():
    from tcs_mi355 import synth
    from tcs_mi355.harness import run_sequence
    seq = synth.make_sequence(3, n_frames=3, height=64, width=96, max_disp=16.0)
    calls = []

    def fake(im1, im2, iters, test_mode, params):
        calls.append((test_mode, torch.is_grad_enabled(), params is None))
        B, _, H, W = im1.shape
        # iteration k predicts -(k+1) everywhere (negative disparity; one positive value checks the clip)
        preds = []
        for k in range(iters):
            a = torch.full((B, 1, H, W), -float(k + 1))
            b = a.clone()
            b[..., 0, 0] = 5.0
            preds.append([a - 1, b])
        h, w = H // 4, W // 4
        return {"flow_predictions": preds, "flow_q_predictions": [[torch.zeros(B, 1, h, w)] * 2] * iters,
                "flow_q": torch.zeros(B, 1, h, w), "net_list": [torch.zeros(B, 8, h, w)], "fmap1": torch.zeros(B, 8, h, w)}

    st = run_sequence(fake, seq, iters=3, device="cpu", per_iteration=True)
    assert [c[0] for c in calls] == [False] * 3 and not any(c[1] for c in calls)
    assert [c[2] for c in calls] == [True, False, False]
    assert len(st.frames) == len(st.per_iteration) == 3
    assert all(len(c) == 3 for c in st.per_iteration)
    for f, fr in zip(range(3), seq.frames):
        gt = torch.as_tensor(fr.disp_gt)
        for k in range(3):
            pr = torch.full_like(gt, float(k + 1))
            pr[..., 0, 0] = 0.0                         # the +5 is clipped to 0
            valid = gt.abs() < 192
            assert st.per_iteration[f][k].epe == pytest.approx(float((pr - gt).abs()[valid].mean()), rel=1e-6)
        assert st.frames[f] == st.per_iteration[f][-1]
    assert st.iteration_epe().shape == (3,)
    assert st.iteration_epe()[0] == pytest.approx(np.mean([c[0].epe for c in st.per_iteration]))
