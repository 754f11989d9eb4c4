"""TCStereo.forward(test_mode=False) on the MI355X: the pair upsampling and scaled resize kernels, every key of the training-output
dict against the reference (tests/golden/train_outputs.npz, tools/make_goldens_train.py), bit-equality with test mode, and the
combinations with the other modes (mixed batches, fp16, prefetch, eager launches)."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import T, epe

pytestmark = pytest.mark.gpu

DICT_KEYS = {"flow_mono", "flow_init", "flow_predictions", "flow_q_predictions", "disp_grad_q_predictions", "cost_volume", "flow_q",
             "net_list", "fmap1"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from tcs_mi355 import native
    native.lib()
    return torch.device("cuda:0")


def _model(dev, W, **kw):
    from core.tc_stereo import TCStereo
    args = Namespace(hidden_dims=[128] * 3, shared_backbone=True, corr_levels=4, corr_radius=4, n_downsample=2, context_norm="none",
                     slow_fast_gru=False, n_gru_layers=3, mixed_precision=False, init_thres=0.5, **kw)
    m = TCStereo(args)
    m.load_state_dict(W, strict=True)
    m = m.to(dev).eval()
    m._pipeline().strict = True                      # a failed capture is an error here, not an eager fall-back
    return m


@pytest.fixture(scope="module")
def model(dev, synth_weights):
    return _model(dev, synth_weights)


@pytest.fixture(scope="module")
def det_model(dev, synth_weights):
    return _model(dev, synth_weights, hip_deterministic=True)


@pytest.fixture(scope="module")
def golden():
    import os
    from conftest import GOLDEN
    return dict(np.load(os.path.join(GOLDEN, "train_outputs.npz")))


@pytest.fixture(scope="module")
def seq():
    from tcs_mi355 import synth
    return synth.make_sequence(7, n_frames=2, height=128, width=160, max_disp=48.0)


def D(x, dev):
    return (x if torch.is_tensor(x) else T(x)).to(dev).contiguous()


def _images(seq, t, dev):
    fr = seq.frames[t]
    return D(fr.image1, dev)[None], D(fr.image2, dev)[None]


def _params(seq, t, prev, dev, **extra):
    """Temporal params of frame t (> 0) from the previous frame's output dict."""
    return dict(K=D(seq.K, dev).float()[None], T=D(seq.frames[t].T, dev)[None], previous_T=D(seq.frames[t - 1].T, dev)[None],
                baseline=torch.tensor([seq.baseline], dtype=torch.float32, device=dev), last_disp=prev["flow_q"],
                last_net_list=prev["net_list"], fmap1=prev["fmap1"], **extra)


def _train(m, im1, im2, iters, params=None):
    with torch.no_grad():
        return m(im1, im2, iters=iters, params=params, test_mode=False)


def _same_as_test_mode(o_train, o_test):
    """The final entries of a training-output dict against the test-mode dict of the same frame, bit for bit."""
    assert torch.equal(torch.clip(o_train["flow_predictions"][-1][1], max=0), o_test["flow"])
    assert torch.equal(o_train["flow_q"], o_test["flow_q"])
    assert torch.equal(o_train["fmap1"], o_test["fmap1"])
    assert all(torch.equal(a, b) for a, b in zip(o_train["net_list"], o_test["net_list"]))


# ------------------------------------------------------------------------------------------------
# kernels
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("hw", [(32, 40), (120, 160), (29, 37)])
def test_pair_kernel_bit_equal_to_two_single_upsamplings(dev, B, hw):
    from tcs_mi355 import ops
    H, W = hw
    gen = torch.Generator().manual_seed(H * W + B)
    da = (torch.rand(B, 1, H, W, generator=gen) * 40 - 2).to(dev)
    db = (da.cpu() + torch.randn(B, 1, H, W, generator=gen)).to(dev)
    mask = torch.randn(B, 144, H, W, generator=gen) * 3
    pick = torch.rand(B, 144, H, W, generator=gen)
    mask[pick < 0.02] = 80.0                        # saturated logits: the softmax's max subtraction matters
    mask[pick > 0.98] = -80.0
    mask = mask.to(dev)
    up_a, q_a = ops.convex_upsample(da, mask, clip=False)
    up_b, q_b = ops.convex_upsample(db, mask, clip=False)
    got = ops.convex_upsample_pair(da, db, mask)
    for x, y in zip(got, (up_a, up_b, q_a, q_b)):
        assert torch.equal(x, y)
    # into slots of stacked tensors, as the loop uses it
    up = torch.full((3, 2, B, 1, 4 * H, 4 * W), float("nan"), device=dev)
    q = torch.full((3, 2, B, 1, H, W), float("nan"), device=dev)
    ops.convex_upsample_pair(da, db, mask, up[1, 0], up[1, 1], q[1, 0], q[1, 1])
    torch.cuda.synchronize()
    assert torch.equal(up[1, 0], up_a) and torch.equal(up[1, 1], up_b) and torch.equal(q[1, 0], q_a) and torch.equal(q[1, 1], q_b)
    assert torch.isnan(up[0]).all() and torch.isnan(up[2]).all() and torch.isnan(q[0]).all() and torch.isnan(q[2]).all()


@pytest.mark.parametrize("shape", [(1, 1, 32, 40), (2, 1, 29, 37), (2, 3, 8, 9)])
def test_scaled_resize_bit_equal_to_scaled_resize(dev, shape):
    from tcs_mi355 import ops
    B, C, H, W = shape
    x = torch.randn(shape, generator=torch.Generator().manual_seed(H * W)).to(dev) * 30
    ref = ops.resize_bilinear(x, 4 * H, 4 * W)
    got = ops.resize_bilinear(x, 4 * H, 4 * W, scale=-4.0)
    assert torch.equal(got, -4 * ref)


# ------------------------------------------------------------------------------------------------
# the model against the reference
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_training_outputs_vs_reference_golden(dev, model, golden, seq, graph):
    model.use_hip_graph = graph
    try:
        iters = int(golden["iters"])
        prev = None
        for t in range(2):
            im1, im2 = _images(seq, t, dev)
            o = _train(model, im1, im2, iters, None if prev is None else _params(seq, t, prev, dev))
            assert set(o) == DICT_KEYS
            p = f"f{t}_"
            # (the golden holds full-resolution maps and the cost volume at sampled flat indices: tools/make_goldens_train.py)
            idx_up, idx_cv = (torch.from_numpy(golden[k]).long().to(dev) for k in ("idx_up", "idx_cv"))
            assert len(o["flow_predictions"]) == len(o["flow_q_predictions"]) == iters
            for k in range(iters):
                for j in range(2):
                    assert tuple(o["flow_predictions"][k][j].shape) == (1, 1, 128, 160)
                    assert epe(o["flow_predictions"][k][j].reshape(-1)[idx_up], golden[p + "flow_predictions"][k, j]) <= 1e-4, (t, k, j)
                    assert tuple(o["flow_q_predictions"][k][j].shape) == golden[p + "flow_q_predictions"].shape[2:]
                    assert epe(o["flow_q_predictions"][k][j], golden[p + "flow_q_predictions"][k, j]) <= 1e-4, (t, k, j)
            assert len(o["disp_grad_q_predictions"]) == iters
            for k in range(iters):
                assert epe(o["disp_grad_q_predictions"][k], golden[p + "disp_grad_q_predictions"][k]) <= 1e-4, (t, k)
            assert tuple(o["cost_volume"].shape) == (1, 40, 32, 40)
            assert epe(o["cost_volume"].reshape(-1)[idx_cv], golden[p + "cost_volume"]) <= 1e-5, t
            for name in ("flow_mono", "flow_init"):
                assert tuple(o[name].shape) == (1, 1, 128, 160)
                assert epe(o[name].reshape(-1)[idx_up], golden[p + name]) <= 1e-4, (t, name)
            assert epe(o["flow_q"], golden[p + "flow_q"]) <= 1e-4, t
            prev = o
    finally:
        model.use_hip_graph = True


# ------------------------------------------------------------------------------------------------
# the same bits as test mode
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_first_frame_bit_equal_to_test_mode(dev, model, seq, graph):
    model.use_hip_graph = graph
    try:
        im1, im2 = _images(seq, 0, dev)
        with torch.no_grad():
            o_test = model(im1, im2, iters=4, test_mode=True)
        o_train = _train(model, im1, im2, 4)
        _same_as_test_mode(o_train, o_test)
        assert torch.equal(o_train["flow_q"], torch.clip(o_train["flow_q_predictions"][-1][1], max=0))
    finally:
        model.use_hip_graph = True


def test_temporal_frame_bit_equal_to_test_mode_deterministic(dev, det_model, seq):
    im1, im2 = _images(seq, 0, dev)
    with torch.no_grad():
        first = det_model(im1, im2, iters=4, test_mode=True)
        im1, im2 = _images(seq, 1, dev)
        o_test = det_model(im1, im2, iters=4, params=_params(seq, 1, first, dev), test_mode=True)
    o_train = _train(det_model, im1, im2, 4, _params(seq, 1, first, dev))
    _same_as_test_mode(o_train, o_test)


# ------------------------------------------------------------------------------------------------
# combinations
# ------------------------------------------------------------------------------------------------
def _finite(o):
    return all(bool(torch.isfinite(t).all()) for t in _flat(o))


def test_mixed_batch(dev, det_model, seq):
    im1, im2 = _images(seq, 0, dev)
    with torch.no_grad():
        first = det_model(im1, im2, iters=4, test_mode=True)
    n1, n2 = _images(seq, 1, dev)
    b1, b2 = torch.cat([im1, n1]), torch.cat([im2, n2])
    prev = {"flow_q": first["flow_q"].repeat(2, 1, 1, 1), "net_list": [t.repeat(2, 1, 1, 1) for t in first["net_list"]],
            "fmap1": first["fmap1"].repeat(2, 1, 1, 1)}
    params = _params(seq, 1, prev, dev, new_sequence=[True, False])
    params.update(K=params["K"].repeat(2, 1, 1), T=params["T"].repeat(2, 1, 1), previous_T=params["previous_T"].repeat(2, 1, 1),
                  baseline=params["baseline"].repeat(2))
    with torch.no_grad():
        o_test = det_model(b1, b2, iters=4, params=params, test_mode=True)
    o_train = _train(det_model, b1, b2, 4, params)
    assert _finite(o_train)
    _same_as_test_mode(o_train, o_test)


def test_fp16_mode(dev, synth_weights, seq):
    m = _model(dev, synth_weights, hip_precision="fp16")
    im1, im2 = _images(seq, 0, dev)
    with torch.no_grad():
        o_test = m(im1, im2, iters=4, test_mode=True)
    o_train = _train(m, im1, im2, 4)
    assert _finite(o_train)
    _same_as_test_mode(o_train, o_test)


def test_prefetch_changes_nothing(dev, model, seq):
    im1, im2 = _images(seq, 0, dev)
    ref = _train(model, im1, im2, 4)
    with torch.no_grad():
        model.prefetch(im1, im2, first=True)         # features without the cost volume: not consumed by the next call
    o = _train(model, im1, im2, 4)
    assert torch.equal(o["cost_volume"], ref["cost_volume"])
    assert torch.equal(o["flow_mono"], ref["flow_mono"]) and torch.equal(o["flow_init"], ref["flow_init"])
    for k in range(4):
        assert all(torch.equal(a, b) for a, b in zip(o["flow_predictions"][k], ref["flow_predictions"][k]))
        assert all(torch.equal(a, b) for a, b in zip(o["flow_q_predictions"][k], ref["flow_q_predictions"][k]))
        assert torch.equal(o["disp_grad_q_predictions"][k], ref["disp_grad_q_predictions"][k])


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_second_call_leaves_first_outputs_untouched(dev, model, seq, graph):
    model.use_hip_graph = graph
    try:
        im1, im2 = _images(seq, 0, dev)
        o1 = _train(model, im1, im2, 4)
        snap = [t.clone() for t in _flat(o1)]
        n1, n2 = _images(seq, 1, dev)
        o2 = _train(model, n1, n2, 4)                                  # a first frame of other images
        _train(model, n1, n2, 4, _params(seq, 1, o1, dev))           # and a temporal frame reading o1
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(_flat(o1), snap))
        assert o1["flow_predictions"][0][0].data_ptr() != o2["flow_predictions"][0][0].data_ptr()
    finally:
        model.use_hip_graph = True


def _flat(o):
    return [o["flow_mono"], o["flow_init"], o["cost_volume"], o["flow_q"], o["fmap1"], *o["net_list"], *o["disp_grad_q_predictions"],
            *[x for p in o["flow_predictions"] for x in p], *[x for p in o["flow_q_predictions"] for x in p]]
