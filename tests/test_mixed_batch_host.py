"""Mixed batches on the host side (no GPU): the *_mixed C ABI symbols, the validation of params["new_sequence"], a numpy restatement of
the masked metric mean and of the prior selection (what tests/test_gpu_mixed_batch.py holds the kernels to), and the continuous-batching
harness `run_sequences` against a deterministic CPU stub model whose output depends on the images and on the threaded state."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

NEW_SYMBOLS = ("tcs_pose_prepare_mixed", "tcs_warp_forward_mixed", "tcs_warp_forward_ordered_mixed", "tcs_bilinear_sample_mixed")


def test_mixed_symbols_exported_and_abi_version():
    from tcs_mi355 import native
    L = native.lib()
    assert L.tcs_abi_version() >= 11
    for name in NEW_SYMBOLS:
        assert name in native.SIGNATURES, name
        assert hasattr(L, name), name


# ------------------------------------------------------------------------------------------------
# params["new_sequence"]
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [
    torch.tensor([True, False, True]),                       # wrong length
    [True, False, False],                                    # wrong length (sequence)
    torch.zeros(2, 2, dtype=torch.bool),                     # 2-D
    [[True], [False]],                                       # nested sequence
    torch.tensor([1.0, 0.0]),                                # float dtype
    torch.tensor([1, 0], dtype=torch.int64),                 # int64 dtype
    [1.0, 0.0],                                              # float elements
    "ab",
    True,                                                    # a scalar is not a [B] mask
])
def test_new_sequence_validation_rejects(value):
    from core.tc_stereo import sequence_starts
    with pytest.raises(ValueError):
        sequence_starts(value, 2)


@pytest.mark.parametrize("value", [torch.tensor([True, False]), torch.tensor([1, 0], dtype=torch.uint8), [True, False],
                                   (True, False), np.array([True, False])])
def test_new_sequence_normalised(value):
    from core.tc_stereo import sequence_starts
    t = sequence_starts(value, 2, torch.device("cpu"))
    assert t.dtype == torch.uint8 and t.shape == (2,) and t.is_contiguous()
    assert t.tolist() == [1, 0]


# ------------------------------------------------------------------------------------------------
# numpy restatement: masked mean, prior selection
# ------------------------------------------------------------------------------------------------
def block_partials(cur_disp, start):
    """k_warp_geometry's per-block partial sums [B, nb] of cur_disp [B,H,W] in float32: 256 pixels per block as four wave sums
    (a butterfly over 64 lanes), combined (w0 + w1) + (w2 + w3); a start element's partials are exact zeros."""
    B = cur_disp.shape[0]
    flat = cur_disp.reshape(B, -1).astype(np.float32)
    n = flat.shape[1]
    nb = -(-n // 256)
    pad = np.zeros((B, nb * 256), np.float32)
    pad[:, :n] = flat
    pad[np.asarray(start, bool)] = 0.0
    w = pad.reshape(B, nb, 4, 64)
    for off in (32, 16, 8, 4, 2, 1):                # the tree order does not matter for the test's tolerance; zeros stay exact
        w = w[..., :off] + w[..., off:2 * off]
    w = w[..., 0]
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def masked_mean(cur_disp, start):
    """The metric mean of a mixed batch: over the temporal elements' pixels only, 0 without a temporal element (no 0/0)."""
    start = np.asarray(start, bool)
    count = int((~start).sum()) * cur_disp[0].size
    total = np.float32(block_partials(cur_disp, start).sum(dtype=np.float32))
    return np.float32(0.0) if count == 0 else np.float32(total * (np.float32(1.0) / np.float32(count)))


def select_prior(warped, prior, start):
    """Per-element selection of (disp, mask, cost): the prior for start elements, the warp's outputs for the others."""
    s = np.asarray(start, bool).reshape(-1, 1, 1, 1)
    return tuple(np.where(s, p, w) for w, p in zip(warped, prior))


def test_masked_mean_restatement():
    rng = np.random.default_rng(0)
    cd = (rng.random((4, 17, 23)) * 40).astype(np.float32)
    start = [True, False, True, False]
    m = masked_mean(cd, start)
    want = cd[[1, 3]].astype(np.float64).mean()
    assert abs(float(m) - want) <= 1e-5 * want
    # = the plain mean of the temporal sub-batch
    assert abs(float(m) - float(masked_mean(cd[[1, 3]], [False, False]))) <= 1e-5 * want
    # a start element's content does not matter, NaN included
    poisoned = cd.copy()
    poisoned[0] = np.nan
    poisoned[2] = 1e30
    assert masked_mean(poisoned, start) == m
    # all temporal: the whole batch; all start: 0, no 0/0
    assert abs(float(masked_mean(cd, [False] * 4)) - cd.astype(np.float64).mean()) <= 1e-5 * cd.mean()
    with np.errstate(all="raise"):
        assert masked_mean(cd, [True] * 4) == 0.0


def test_prior_selection_restatement():
    rng = np.random.default_rng(1)
    shape = (3, 1, 5, 6)
    warped = [rng.random(shape).astype(np.float32) for _ in range(3)]
    prior = [rng.random(shape).astype(np.float32) for _ in range(3)]
    warped[0][0] = np.nan
    got = select_prior(warped, prior, [True, False, True])
    for g, w, p in zip(got, warped, prior):
        assert np.array_equal(g[0], p[0]) and np.array_equal(g[1], w[1]) and np.array_equal(g[2], p[2])
    all_start = select_prior(warped, prior, [True] * 3)
    assert all(np.array_equal(g, p) for g, p in zip(all_start, prior))


# ------------------------------------------------------------------------------------------------
# run_sequences against a CPU stub
# ------------------------------------------------------------------------------------------------
H, W = 20, 28          # padded to 32 x 32


def make_seq(sid, n):
    rng = np.random.default_rng(100 + sid)
    frames = []
    for f in range(n):
        im1 = (rng.random((3, H, W)) * 255).astype(np.float32)
        im2 = (rng.random((3, H, W)) * 255).astype(np.float32)
        im1[0, 0, 0] = 1000.0 * (sid + 1) + f                   # the stub reads (sequence, frame) from here
        T = np.eye(4, dtype=np.float32)
        T[0, 3] = 0.1 * f + 0.01 * sid
        gt = (rng.random((1, H, W)) * 20).astype(np.float32)
        frames.append(SimpleNamespace(image1=im1, image2=im2, disp_gt=gt, T=T))
    K = np.array([[50.0 + sid, 0, W / 2], [0, 50.0, H / 2], [0, 0, 1]], np.float32)
    return SimpleNamespace(frames=frames, K=K, baseline=0.2 + 0.01 * sid)


class Stub:
    """A deterministic batch model: each element's output depends on its images and, on a temporal element, on every entry of its
    threaded state (last_disp, last_net_list, fmap1, previous_T, K).  A start element (params=None, or new_sequence True) reads no
    state.  Records (sequence, frame, start) per element; zero images are the harness's padding."""

    def __init__(self):
        self.calls = []

    def __call__(self, im1, im2, iters=12, test_mode=True, params=None):
        from core.tc_stereo import sequence_starts
        B = im1.shape[0]
        if params is None:
            start = [True] * B
        elif params.get("new_sequence") is None:
            start = [False] * B
        else:
            start = [bool(v) for v in sequence_starts(params["new_sequence"], B).tolist()]
        rec = []
        for b in range(B):
            code = float(im1[b, 0, 0, 0])
            rec.append(("pad", None, start[b]) if code == 0.0 and float(im1[b].abs().sum()) == 0.0
                       else (int(code // 1000) - 1, int(code % 1000), start[b]))
        self.calls.append(rec)
        now = F.avg_pool2d(im1.mean(1, keepdim=True) - 0.5 * im2.mean(1, keepdim=True), 4) / 10.0
        q = []
        for b in range(B):
            x = now[b:b + 1]
            if not start[b]:
                p = params
                x = x + 0.5 * p["last_disp"][b:b + 1] + 0.25 * p["fmap1"][b:b + 1].mean() + 0.125 * p["last_net_list"][1][b:b + 1].mean() \
                    + p["previous_T"][b, 0, 3] + 0.001 * p["K"][b, 0, 0] + p["baseline"][b]
                assert torch.isfinite(x).all()
            q.append(x)
        flow_q = torch.cat(q, 0)
        return {"flow": -F.interpolate(flow_q, scale_factor=4, mode="nearest"), "flow_q": flow_q,
                "net_list": [flow_q * 2, flow_q * 3], "fmap1": flow_q + 1}


LENGTHS = [3, 1, 6, 2, 4]


def test_run_sequences_matches_run_sequence_for_any_order():
    from tcs_mi355.harness import run_sequence, run_sequences
    seqs = [make_seq(i, n) for i, n in enumerate(LENGTHS)]
    single = [run_sequence(Stub(), q, iters=2, device="cpu") for q in seqs]
    for perm in [list(range(5)), [4, 3, 2, 1, 0], [2, 0, 4, 1, 3]]:
        stub = Stub()
        got = run_sequences(stub, [seqs[i] for i in perm], iters=2, device="cpu", batch=3)
        assert len(got) == 5
        for k, i in enumerate(perm):                       # stats in input order, equal to run_sequence's
            assert len(got[k].frames) == LENGTHS[i]
            for a, b in zip(got[k].frames, single[i].frames):
                assert a.epe == pytest.approx(b.epe, rel=1e-6, abs=1e-7)
                assert a.d1_weighted == pytest.approx(b.d1_weighted, rel=1e-6, abs=1e-7)
                assert a.d3_weighted == pytest.approx(b.d3_weighted, rel=1e-6, abs=1e-7)
                assert a.mask_rate == b.mask_rate
        # the schedule: every call is 3 wide; new_sequence is True exactly on a sequence's first frame (and on padding)
        seen = {}
        pads = 0
        for call in stub.calls:
            assert len(call) == 3
            for sid, f, st in call:
                if sid == "pad":
                    pads += 1
                    assert st
                    continue
                assert st == (f == 0), (sid, f, st)
                seen.setdefault(sid, []).append(f)
        assert pads > 0
        # every frame of every sequence exactly once, in order; padding never counted
        assert sorted(seen) == list(range(5))
        for sid, fs in seen.items():
            assert fs == list(range(len(fs)))
        assert sum(len(fs) for fs in seen.values()) == sum(LENGTHS) == sum(len(s.frames) for s in got)
        assert len(stub.calls) * 3 == sum(LENGTHS) + pads


def test_run_sequences_collect_and_errors():
    from tcs_mi355.harness import run_sequence, run_sequences
    seqs = [make_seq(i, n) for i, n in enumerate([2, 3])]
    got = []
    run_sequences(Stub(), seqs, iters=1, device="cpu", batch=4, collect=got)
    assert [len(g) for g in got] == [2, 3]
    for q, g in zip(seqs, got):
        alone = []
        run_sequence(Stub(), q, iters=1, device="cpu", collect=alone)
        for a, b in zip(g, alone):
            assert a.shape == b.shape == (1, 1, H, W)
            assert torch.allclose(a, b, rtol=1e-6, atol=1e-6)
    other = make_seq(9, 2)
    for fr in other.frames:
        fr.image1 = np.zeros((3, 40, W), np.float32)
        fr.image2 = np.zeros((3, 40, W), np.float32)
    with pytest.raises(ValueError):
        run_sequences(Stub(), seqs + [other], iters=1, device="cpu", batch=2)
    with pytest.raises(ValueError):
        run_sequences(Stub(), seqs, iters=1, device="cpu", batch=2, prefetch=True)


def test_run_sequences_without_temporal_state():
    """temporal=False: every call is params=None (every element a first frame), like run_sequence(temporal=False)."""
    from tcs_mi355.harness import run_sequence, run_sequences
    seqs = [make_seq(i, n) for i, n in enumerate([2, 4, 1])]
    stub = Stub()
    got = run_sequences(stub, seqs, iters=1, device="cpu", batch=2, temporal=False)
    assert all(st for call in stub.calls for _, _, st in call)
    for q, g in zip(seqs, got):
        want = run_sequence(Stub(), q, iters=1, device="cpu", temporal=False)
        assert [f.epe for f in g.frames] == pytest.approx([f.epe for f in want.frames], rel=1e-6)

