"""Mixed batches on the MI355X: independent sequences on the batch dimension that start at different frames (params["new_sequence"]).
The kernels (tcs_*_mixed) against a float64 restatement and against the existing entry points, the model's mixed path against the
first-frame and temporal paths and against each element run alone, poisoned state of the start elements, one REFINE capture for every
mask pattern, and the continuous-batching harness (tcs_mi355.harness.run_sequences) against run_sequence."""
import numpy as np
import pytest
import torch

from conftest import epe
from test_gpu_deterministic import _model, _warp_case, _warp_f64, _check

pytestmark = pytest.mark.gpu

H, W, ITERS = 96, 128, 3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from tcs_mi355 import native
    native.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def atomic_model(dev, synth_weights):
    return _model(dev, synth_weights)


@pytest.fixture(scope="module")
def det_model(dev, synth_weights):
    return _model(dev, synth_weights, hip_deterministic=True)


def D(x, dev):
    return (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))).to(dev).contiguous()


def _frame(seq, t, dev):
    """(image1, image2, K, T, baseline) of frame t of a synthetic sequence, padded as the harness pads it, batch 1."""
    from tcs_mi355.harness import InputPadder
    fr = seq.frames[t]
    im1, im2 = D(fr.image1, dev)[None], D(fr.image2, dev)[None]
    padder = InputPadder(im1.shape, divis_by=32)
    (im1, im2), K = padder.pad(im1, im2, K=D(seq.K, dev).float()[None])
    return im1, im2, K, D(fr.T, dev)[None], torch.tensor([seq.baseline], dtype=torch.float32, device=dev)


def _stack(frames):
    return [torch.cat(xs, 0) for xs in zip(*frames)]


def _clone(o):
    return {"flow": o["flow"].clone(), "flow_q": o["flow_q"].clone(), "net_list": [t.clone() for t in o["net_list"]],
            "fmap1": o["fmap1"].clone()}


def _params(state, K, T, base, **extra):
    """state = (previous output, previous T)."""
    o, Tp = state
    return dict(K=K, T=T, previous_T=Tp, baseline=base, last_disp=o["flow_q"], last_net_list=o["net_list"], fmap1=o["fmap1"], **extra)


def _equal(a, b):
    return (torch.equal(a["flow"], b["flow"]) and torch.equal(a["flow_q"], b["flow_q"]) and torch.equal(a["fmap1"], b["fmap1"])
            and all(torch.equal(x, y) for x, y in zip(a["net_list"], b["net_list"])))


def _sub(o, b):
    return {"flow": o["flow"][b:b + 1], "flow_q": o["flow_q"][b:b + 1], "fmap1": o["fmap1"][b:b + 1],
            "net_list": [t[b:b + 1] for t in o["net_list"]]}


@pytest.fixture(scope="module")
def seqs():
    from tcs_mi355 import synth
    return [synth.make_sequence(60 + j, n_frames=3, height=H, width=W, max_disp=32.0) for j in range(4)]


def _two_frames(model, seqs, dev, idx):
    """Frame 0 (params=None) of the sequences `idx` as one batch, and frame 1's inputs."""
    f0 = _stack([_frame(seqs[i], 0, dev) for i in idx])
    f1 = _stack([_frame(seqs[i], 1, dev) for i in idx])
    o0 = _clone(model(f0[0], f0[1], iters=ITERS, test_mode=True))
    return (o0, f0[3]), f0, f1


# ------------------------------------------------------------------------------------------------
# 1-2: the mixed path against the first-frame and the temporal paths
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_all_true_is_bit_equal_to_first_frame(dev, atomic_model, seqs, graph):
    m = atomic_model
    m.use_hip_graph = graph
    try:
        state, _, f1 = _two_frames(m, seqs, dev, [0, 1])
        im1, im2, K, T, base = f1
        first = _clone(m(im1, im2, iters=ITERS, test_mode=True))
        for mask in (torch.ones(2, dtype=torch.bool, device=dev), [True, True], torch.ones(2, dtype=torch.uint8)):
            mixed = _clone(m(im1, im2, iters=ITERS, test_mode=True, params=_params(state, K, T, base, new_sequence=mask)))
            assert _equal(mixed, first)
    finally:
        m.use_hip_graph = None


def test_all_false_equals_temporal(dev, atomic_model, det_model, seqs):
    for m, exact in ((det_model, True), (atomic_model, False)):
        state, _, f1 = _two_frames(m, seqs, dev, [0, 1])
        im1, im2, K, T, base = f1
        temporal = _clone(m(im1, im2, iters=ITERS, test_mode=True, params=_params(state, K, T, base)))
        mixed = _clone(m(im1, im2, iters=ITERS, test_mode=True,
                         params=_params(state, K, T, base, new_sequence=torch.zeros(2, dtype=torch.bool, device=dev))))
        if exact:
            assert _equal(mixed, temporal)
        else:
            assert epe(mixed["flow"], temporal["flow"]) <= 1e-5


# ------------------------------------------------------------------------------------------------
# 3: a mixed batch against each element alone
# ------------------------------------------------------------------------------------------------
def _mixed_vs_alone(m, seqs, dev):
    """B=4: elements 0 and 2 start sequences 2 / 3 (frame 0), elements 1 and 3 continue sequences 1 / 0 (frame 1) -> the largest EPE
    of an element against that element run alone, and whether every element is bit-equal."""
    from tcs_mi355 import synth
    fresh = [synth.make_sequence(80 + j, n_frames=1, height=H, width=W, max_disp=32.0) for j in range(2)]
    state, f0, _ = _two_frames(m, seqs, dev, [2, 1, 3, 0])               # slots run sequences 2, 1, 3, 0 on frame 0
    rows = [_frame(fresh[0], 0, dev), _frame(seqs[1], 1, dev), _frame(fresh[1], 0, dev), _frame(seqs[0], 1, dev)]
    im1, im2, K, T, base = _stack(rows)
    start = torch.tensor([True, False, True, False], device=dev)
    out = _clone(m(im1, im2, iters=ITERS, test_mode=True, params=_params(state, K, T, base, new_sequence=start)))
    worst, exact = 0.0, True
    for b, (kind, q) in enumerate((("start", fresh[0]), ("temporal", seqs[1]), ("start", fresh[1]), ("temporal", seqs[0]))):
        a0 = _frame(q, 0, dev)
        alone = _clone(m(a0[0], a0[1], iters=ITERS, test_mode=True))
        if kind == "temporal":
            a1 = _frame(q, 1, dev)
            alone = _clone(m(a1[0], a1[1], iters=ITERS, test_mode=True, params=_params((alone, a0[3]), a1[2], a1[3], a1[4])))
        got = _sub(out, b)
        worst = max(worst, epe(got["flow"], alone["flow"]))
        exact = exact and _equal(got, alone)
    return worst, exact


@pytest.mark.parametrize("deterministic", [False, True], ids=["atomic", "deterministic"])
def test_mixed_batch_matches_each_element_alone(dev, atomic_model, det_model, seqs, deterministic):
    worst, exact = _mixed_vs_alone(det_model if deterministic else atomic_model, seqs, dev)
    print(f"mixed B=4 vs alone ({'deterministic' if deterministic else 'atomic'}): worst EPE {worst:.3e}, bit-equal {exact}")
    assert worst <= 1e-5, worst


# ------------------------------------------------------------------------------------------------
# 4: poisoned state of the start elements
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", [float("nan"), 1e30], ids=["nan", "1e30"])
def test_start_elements_state_is_never_read(dev, det_model, seqs, poison):
    from tcs_mi355 import s16
    m = det_model
    state, _, f1 = _two_frames(m, seqs, dev, [0, 1, 2, 3])
    im1, im2, K, T, base = f1
    start = torch.tensor([True, False, True, False], device=dev)
    sel = start.view(-1, 1, 1, 1)

    def fill(v):
        o, Tp = state
        f = lambda t: torch.where(sel.view(-1, *([1] * (t.ndim - 1))), torch.full_like(t, v), t)
        return ({"flow": o["flow"], "flow_q": f(o["flow_q"]), "net_list": [f(t) for t in o["net_list"]], "fmap1": f(o["fmap1"])},
                torch.where(sel.view(-1, 1, 1), torch.full_like(Tp, v), Tp))

    s16.take_flags()
    zero = _clone(m(im1, im2, iters=ITERS, test_mode=True, params=_params(fill(0.0), K, T, base, new_sequence=start)))
    bad = _clone(m(im1, im2, iters=ITERS, test_mode=True, params=_params(fill(poison), K, T, base, new_sequence=start)))
    torch.cuda.synchronize()
    assert s16.take_flags() == 0
    for o in (zero, bad):
        assert torch.isfinite(o["flow"]).all() and torch.isfinite(o["flow_q"]).all() and torch.isfinite(o["fmap1"]).all()
        assert all(torch.isfinite(t).all() for t in o["net_list"])
    assert _equal(bad, zero)


# ------------------------------------------------------------------------------------------------
# 5: kernel level
# ------------------------------------------------------------------------------------------------
def _poison_rows(t, start, v=float("nan")):
    t = t.clone()
    t[torch.as_tensor(start, dtype=torch.bool)] = v
    return t


def _integer_warp_case(B, Cc, Hh, Ww, seed):
    """Depths that are powers of two, an identity pose and a power-of-two focal length: every source lands exactly on its own pixel, so
    each target sums one non-zero contribution and the float-atomic splat is order-independent (bit-comparable)."""
    gen = torch.Generator().manual_seed(seed)
    K = torch.tensor([[64.0, 0, 64.0], [0, 64.0, 48.0], [0, 0, 1.0]]).repeat(B, 1, 1)
    Ki = torch.linalg.inv(K.double()).float()
    base = torch.full((B,), 0.25)                                   # baseline * fx = 16
    disp = 16.0 / 2.0 ** torch.randint(0, 5, (B, 1, Hh, Ww), generator=gen).float()
    fm, cur = torch.randn(B, Cc, Hh, Ww, generator=gen), torch.randn(B, Cc, Hh, Ww, generator=gen)
    return disp, fm, cur, torch.eye(4).repeat(B, 1, 1), K, Ki, base


@pytest.mark.parametrize("ordered", [False, True], ids=["atomic", "ordered"])
def test_warp_forward_mixed_kernels(dev, ordered):
    from tcs_mi355 import ops
    B, Cc, Hh, Ww = 4, 37, 33, 45
    disp, fm, cur, Tr, K, Ki, base = _warp_case(B, Cc, Hh, Ww, 11)
    start = [True, False, False, True]
    keep = [b for b in range(B) if not start[b]]
    gen = torch.Generator().manual_seed(12)
    prior = [torch.rand(B, 1, Hh, Ww, generator=gen) * 20, torch.rand(B, 1, Hh, Ww, generator=gen),
             (torch.rand(B, 1, Hh, Ww, generator=gen) > 0.5).float()]
    st = torch.tensor(start, device=dev)
    # start elements' inputs poisoned: never read
    args = [D(_poison_rows(t, start), dev) for t in (disp, fm, Tr, K, Ki, base)]
    od, of, om, oc = ops.warp_forward(*args, cur_fmap=D(cur, dev), ordered=ordered, start=st, prior=[D(p, dev) for p in prior])
    # temporal elements: the reference warp() of the temporal sub-batch, in float64
    ref = _warp_f64(dev, *(t[keep] for t in (disp, fm, cur, Tr, K, Ki, base)))
    for name, t in (("disp", od), ("fmap", of), ("mask", om), ("cost", oc)):
        _check(t[keep], ref[name], name)
    # start elements: the prior, bit for bit, and zero features
    for b in range(B):
        if start[b]:
            assert torch.equal(od[b].cpu(), prior[0][b]) and torch.equal(oc[b].cpu(), prior[1][b]) and torch.equal(om[b].cpu(), prior[2][b])
            assert torch.equal(of[b].cpu(), torch.zeros_like(fm[b]))
    # all start: every output is the prior, no mean formed
    ad, _, am, ac = ops.warp_forward(*args, cur_fmap=D(cur, dev), want_fmap=False, ordered=ordered,
                                     start=torch.ones(B, dtype=torch.uint8, device=dev), prior=[D(p, dev) for p in prior])
    assert torch.equal(ad.cpu(), prior[0]) and torch.equal(ac.cpu(), prior[1]) and torch.equal(am.cpu(), prior[2])
    # all-zero mask: bit-equal to the existing entry point (an order-independent case for the atomic splat)
    case = _integer_warp_case(B, Cc, Hh, Ww, 13) if not ordered else (disp, fm, cur, Tr, K, Ki, base)
    a2 = [D(t, dev) for t in (case[0], case[1], case[3], case[4], case[5], case[6])]
    z = torch.zeros(B, dtype=torch.bool, device=dev)
    want = ops.warp_forward(*a2, cur_fmap=D(case[2], dev), ordered=ordered)
    got = ops.warp_forward(*a2, cur_fmap=D(case[2], dev), ordered=ordered, start=z, prior=[D(p, dev) for p in prior])
    for w, g in zip(want, got):
        assert torch.equal(w, g)


def test_bilinear_sample_and_pose_prepare_mixed(dev):
    from tcs_mi355 import ops
    gen = torch.Generator().manual_seed(7)
    B, C, Hi, Wi, Ho, Wo = 3, 21, 24, 32, 24, 32
    img = torch.randn(B, C, Hi, Wi, generator=gen)
    grid = torch.stack([torch.rand(B, Ho, Wo, generator=gen) * Wi, torch.rand(B, Ho, Wo, generator=gen) * Hi], 1)
    start = [False, True, False]
    st = torch.tensor(start, device=dev)
    want = ops.bilinear_sample(D(img, dev), D(grid, dev))
    got = ops.bilinear_sample(D(_poison_rows(img, start), dev), D(_poison_rows(grid, start), dev), start=st)
    assert torch.equal(got[1].cpu(), torch.zeros(C, Ho, Wo)) and not torch.signbit(got[1]).any()
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])
    # poses: identity T_rel / T_back for the start element, its T / T_prev unread; K_scaled as the non-mixed call
    K = torch.tensor([[320.0, 0, 320.0], [0, 320.0, 240.0], [0, 0, 1.0]]).repeat(B, 1, 1)
    T = torch.eye(4).repeat(B, 1, 1)
    T[:, :3, 3] = torch.randn(B, 3, generator=gen)
    Tp = torch.eye(4).repeat(B, 1, 1)
    Tp[:, :3, 3] = torch.randn(B, 3, generator=gen)
    ref = ops.pose_prepare(D(K, dev), D(T, dev), D(Tp, dev), 0.25)
    mix = ops.pose_prepare(D(K, dev), D(_poison_rows(T, start), dev), D(_poison_rows(Tp, start), dev), 0.25, start=st)
    for r, g in zip(ref, mix):
        assert torch.equal(r[0], g[0]) and torch.equal(r[2], g[2])
    assert torch.equal(mix[0], ref[0]) and torch.equal(mix[1], ref[1])
    assert torch.equal(mix[2][1].cpu(), torch.eye(4)) and torch.equal(mix[3][1].cpu(), torch.eye(4))


# ------------------------------------------------------------------------------------------------
# 6: one REFINE capture for every mask pattern; graph replay = eager
# ------------------------------------------------------------------------------------------------
def test_masks_share_one_capture_and_replay_equals_eager(dev, synth_weights, seqs):
    m = _model(dev, synth_weights, hip_deterministic=True)
    state, _, f1 = _two_frames(m, seqs, dev, [0, 1, 2])
    im1, im2, K, T, base = f1
    before = m._pipeline().captures
    masks = ([True, False, False], [False, True, True], [False, False, False])
    graph = [_clone(m(im1, im2, iters=ITERS, test_mode=True, params=_params(state, K, T, base, new_sequence=torch.tensor(k, device=dev))))
             for k in masks]
    assert m._pipeline().captures == before + 1
    m.use_hip_graph = False
    try:
        eager = [_clone(m(im1, im2, iters=ITERS, test_mode=True, params=_params(state, K, T, base, new_sequence=list(k)))) for k in masks]
    finally:
        m.use_hip_graph = None
    for g, e in zip(graph, eager):
        assert _equal(g, e)
    assert not _equal(graph[0], graph[2])


# ------------------------------------------------------------------------------------------------
# 7: continuous batching
# ------------------------------------------------------------------------------------------------
def test_run_sequences_matches_run_sequence(dev, atomic_model):
    from tcs_mi355 import synth
    from tcs_mi355.harness import run_sequence, run_sequences
    lengths = [3, 5, 2, 4, 2]
    data = [synth.make_sequence(90 + j, n_frames=n, height=H, width=W, max_disp=32.0) for j, n in enumerate(lengths)]
    single = []
    for q in data:
        c = []
        run_sequence(atomic_model, q, iters=ITERS, device=dev, collect=c)
        single.append(c)
    runs = {}
    for pf in (False, True):
        before = atomic_model._pipeline().prefetched
        got = []
        stats = run_sequences(atomic_model, data, iters=ITERS, device=dev, batch=3, collect=got, prefetch=pf)
        if pf:
            assert atomic_model._pipeline().prefetched > before
        assert [len(s.frames) for s in stats] == lengths and [len(g) for g in got] == lengths
        assert all(s.domain_flags == 0 for s in stats)
        for j in range(len(data)):
            for t in range(lengths[j]):
                assert epe(got[j][t], single[j][t]) <= 1e-5, (pf, j, t)
        runs[pf] = got
    for a, b in zip(runs[False], runs[True]):
        for x, y in zip(a, b):
            assert epe(x, y) <= 1e-5


def test_run_sequences_640x480(dev, atomic_model):
    """The real frame size once: two sequences of 2 / 3 frames over batch 2 (a padded tail), 8 iterations."""
    from tcs_mi355 import synth
    from tcs_mi355.harness import run_sequence, run_sequences
    data = [synth.make_sequence(2000 + j, n_frames=n, height=480, width=640, max_disp=192.0) for j, n in enumerate((2, 3))]
    got = []
    run_sequences(atomic_model, data, iters=8, device=dev, batch=2, collect=got)
    for j, q in enumerate(data):
        c = []
        run_sequence(atomic_model, q, iters=8, device=dev, collect=c)
        for t, x in enumerate(c):
            assert epe(got[j][t], x) <= 1e-5, (j, t)
