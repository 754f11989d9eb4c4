"""The opt-in deterministic mode on the MI355X: the ordered splat (tcs_softsplat_sum_ordered, tcs_warp_forward_ordered) bit for bit against
the host float32 restatement of its documented order (tests/test_deterministic_host.py), the ordered warp against float64, run to run
under concurrency, and the model (TCStereo(args) with args.hip_deterministic = True): every frame of a sequence bit-reproducible."""
import math

import numpy as np
import pytest
import torch

from conftest import epe
from test_deterministic_host import edge_flow, scatter_f64, splat_entries, splat_sum_ordered

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from tcs_mi355 import native
    native.lib()
    return torch.device("cuda:0")


def D(x, dev):
    return (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))).to(dev).contiguous()


# ------------------------------------------------------------------------------------------------
# ordered summation splat, bit for bit
# ------------------------------------------------------------------------------------------------
def _single_target_flow(B, H, W, tx, ty):
    """Every source pixel lands at (tx, ty) (fractional: four target lists of H*W entries each)."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    f = np.stack([np.float32(tx) - x, np.float32(ty) - y]).astype(np.float32)
    return np.repeat(f[None], B, axis=0)


SUM_CASES = [
    ("random_b2_odd", 2, 5, 7, 9, lambda B, H, W: (np.random.default_rng(3).standard_normal((B, 2, H, W)) * 3).astype(np.float32)),
    ("edges_b2_odd", 2, 6, 13, 17, lambda B, H, W: edge_flow(B, H, W, 4)),
    ("edges_b1", 1, 37, 33, 45, lambda B, H, W: edge_flow(B, H, W, 5)),
    ("single_target_small_b2", 2, 4, 9, 11, lambda B, H, W: _single_target_flow(B, H, W, 5.25, 3.5)),
    ("single_integer_target", 1, 3, 5, 7, lambda B, H, W: _single_target_flow(B, H, W, 2.0, 2.0)),
    ("single_target_120x160", 1, 3, 120, 160, lambda B, H, W: _single_target_flow(B, H, W, 80.25, 60.75)),
]


@pytest.mark.parametrize("name,B,C,H,W,make", SUM_CASES, ids=[c[0] for c in SUM_CASES])
def test_ordered_sum_splat_equals_restatement(dev, name, B, C, H, W, make):
    from tcs_mi355 import ops
    inp = (np.random.default_rng(len(name)).standard_normal((B, C, H, W)) * 4).astype(np.float32)
    flow = make(B, H, W)
    got = ops.softsplat_sum(D(inp, dev), D(flow, dev), ordered=True)
    want = torch.from_numpy(splat_sum_ordered(inp, flow))
    assert torch.equal(got.cpu(), want), float((got.cpu() - want).abs().max())
    # the atomic path sums the same contributions in another order: both within the fp32 reassociation bound of the float64 sum
    ref, mag, cnt = scatter_f64(inp, flow)
    tol = (cnt + 1) * 2.0 ** -24 * mag
    atomic = ops.softsplat_sum(D(inp, dev), D(flow, dev)).cpu().double().numpy()
    assert np.all(np.abs(atomic - ref) <= tol) and np.all(np.abs(want.double().numpy() - ref) <= tol)


def test_ordered_sum_splat_batch_elements_are_independent(dev):
    from tcs_mi355 import ops
    B, C, H, W = 3, 4, 11, 13
    g = np.random.default_rng(9)
    inp = g.standard_normal((B, C, H, W)).astype(np.float32)
    flow = edge_flow(B, H, W, 9)
    whole = ops.softsplat_sum(D(inp, dev), D(flow, dev), ordered=True).cpu()
    for b in range(B):
        one = ops.softsplat_sum(D(inp[b:b + 1], dev), D(flow[b:b + 1], dev), ordered=True).cpu()
        assert torch.equal(one[0], whole[b]), b


# ------------------------------------------------------------------------------------------------
# ordered warp against float64
# ------------------------------------------------------------------------------------------------
def _warp_case(B, Cc, H, W, seed):
    gen = torch.Generator().manual_seed(seed)
    disp = torch.rand(B, 1, H, W, generator=gen) * 30 + 1
    disp[:, :, :, W // 2:] += 15                                # a depth discontinuity
    fm, cur = torch.randn(B, Cc, H, W, generator=gen), torch.randn(B, Cc, H, W, generator=gen)
    K = torch.tensor([[W / 2.0, 0, W / 2.0], [0, W / 2.0, H / 2.0], [0, 0, 1.0]]).repeat(B, 1, 1)
    Ki = torch.linalg.inv(K)
    Tr = torch.eye(4).repeat(B, 1, 1)
    for b in range(B):
        Tr[b, :3, 3] = torch.tensor([0.03, -0.01, -0.06]) * (1 + b)
        a = 0.02 * (1 - 2 * b)
        Tr[b, :3, :3] = torch.tensor([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    base = torch.full((B,), 0.25)
    return disp, fm, cur, Tr, K, Ki, base


def _warp_f64(dev, disp, fm, cur, Tr, K, Ki, base):
    """float64 restatement at the kernel's own landing positions (ops.warp_geometry) and a per-output bound: every term carries <= 4
    fp32 roundings (expf, two products, the landing weights' own are shared), the sum n more, the division one."""
    from tcs_mi355 import ops
    cd, va, fl, me = (t.cpu().numpy() for t in ops.warp_geometry(*(D(t, dev) for t in (disp, Tr, K, Ki, base))))
    s = np.exp(me.astype(np.float64))
    vals = np.concatenate([fm.numpy(), cd, np.ones_like(cd)], 1)
    acc = splat_sum_ordered(vals, fl, valid=va, scale=s, dtype=np.float64)
    mag = splat_sum_ordered(np.abs(vals), fl, valid=va, scale=s, dtype=np.float64)
    n_max = max(int(np.bincount(splat_entries(fl[b], va[b, 0])[0]).max()) for b in range(fl.shape[0]))
    C = fm.shape[1]
    norm = acc[:, C + 1:]
    den = np.maximum(norm, 1e-7)
    out = acc[:, :C + 1] / den
    gam = (n_max + 6) * 2.0 ** -24
    tol = 2 * (gam * (mag[:, :C + 1] / den + np.abs(out)) + 2.0 ** -23 * np.abs(out))
    mask = (norm != 0).astype(np.float64)
    od, of = out[:, C:C + 1], out[:, :C]
    c = cur.numpy().astype(np.float64)
    n1, nw = np.sqrt((c * c).sum(1, keepdims=True)), np.sqrt((of * of).sum(1, keepdims=True))
    cos = (c * of).sum(1, keepdims=True) / (np.maximum(n1, 1e-12) * np.maximum(nw, 1e-12)) * mask
    dfw = np.sqrt((tol[:, :C] ** 2).sum(1, keepdims=True))
    tol_cos = 2 * dfw / np.maximum(nw, 1e-12) + 4 * C * 2.0 ** -24
    return dict(disp=(od, tol[:, C:C + 1]), fmap=(of, tol[:, :C]), mask=(mask, np.zeros_like(mask)), cost=(cos, tol_cos))


def _check(got, ref, what):
    want, tol = ref
    err = np.abs(got.detach().cpu().double().numpy() - want)
    assert np.all(err <= tol), (what, float(np.max(err - tol)))


@pytest.mark.parametrize("B,Cc,H,W,seed", [(1, 256, 120, 160, 5), (2, 37, 33, 45, 6)])
def test_ordered_warp_vs_float64_and_atomic(dev, B, Cc, H, W, seed):
    from tcs_mi355 import ops
    case = _warp_case(B, Cc, H, W, seed)
    disp, fm, cur, Tr, K, Ki, base = case
    args = [D(t, dev) for t in (disp, fm, Tr, K, Ki, base)]
    ref = _warp_f64(dev, *case)
    wd, wf, wm, wc = ops.warp_forward(*args, cur_fmap=D(cur, dev), ordered=True)
    for name, t in (("disp", wd), ("fmap", wf), ("mask", wm), ("cost", wc)):
        _check(t, ref[name], name)
    ad, af, am, ac = ops.warp_forward(*args, cur_fmap=D(cur, dev))
    for name, t in (("disp", ad), ("fmap", af), ("mask", am), ("cost", ac)):
        _check(t, ref[name], "atomic " + name)
    # want_fmap=False / no cost: the same disparity and mask
    d2, f2, m2, c2 = ops.warp_forward(*args, want_fmap=False, ordered=True)
    assert f2 is None and c2 is None and torch.equal(d2, wd) and torch.equal(m2, wm)


# ------------------------------------------------------------------------------------------------
# run to run
# ------------------------------------------------------------------------------------------------
def test_ordered_warp_is_bit_identical_run_to_run_and_under_concurrency(dev):
    from tcs_mi355 import ops, s16
    disp, fm, cur, Tr, K, Ki, base = _warp_case(1, 256, 120, 160, 7)
    args = [D(t, dev) for t in (disp, fm, Tr, K, Ki, base)]
    curd = D(cur, dev)

    def run():
        return ops.warp_forward(*args, cur_fmap=curd, ordered=True)

    ref = [t.clone() for t in run()]
    torch.cuda.synchronize()

    def same(outs):
        return all(torch.equal(a, b) for a, b in zip(outs, ref))

    for _ in range(4):
        assert same(run())
    # two streams at once
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    res = []
    for _ in range(4):
        with torch.cuda.stream(sa):
            ra = run()
        with torch.cuda.stream(sb):
            rb = run()
        res.append((ra, rb))
    torch.cuda.synchronize()
    assert all(same(ra) and same(rb) for ra, rb in res)
    # beside an MFMA convolution that loops on another stream (the pattern of test_stem7x7_beside_concurrent_kernels)
    gen = torch.Generator().manual_seed(0)
    R = lambda *sh: torch.randn(*sh, generator=gen).to(dev)
    pca = ops.pack_conv(R(256, 128, 3, 3) * 0.03, R(256) * 0.1, "f16x3")
    xa, oa = s16.to_s16(R(1, 128, 120, 160)), s16.zeros(1, 256, 120, 160, dev)
    torch.cuda.synchronize()
    bad = torch.zeros((), dtype=torch.int64, device=dev)
    for _ in range(20):
        with torch.cuda.stream(sb):
            for _ in range(3):
                s16.conv2d(pca, [xa], out16=oa)
        with torch.cuda.stream(sa):
            outs = run()
            for a, b in zip(outs, ref):
                bad += (a != b).any().long()
    torch.cuda.synchronize()
    assert int(bad) == 0


# ------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------
def _model(dev, weights, **over):
    from argparse import Namespace
    from core.tc_stereo import TCStereo
    a = dict(hidden_dims=[128] * 3, shared_backbone=True, corr_levels=4, corr_radius=4, n_downsample=2, context_norm="none",
             slow_fast_gru=False, n_gru_layers=3, mixed_precision=False, init_thres=0.5)
    a.update(over)
    m = TCStereo(Namespace(**a))
    m.load_state_dict(weights, strict=True)
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def det_model(dev, synth_weights):
    m = _model(dev, synth_weights, hip_deterministic=True)
    assert m.hip_deterministic
    return m


def _free_run(model, seq, iters, dev):
    """The clip frame by frame as evaluate_stereo.py threads it (tcs_mi355.harness.run_sequence), keeping every frame's full output."""
    from tcs_mi355 import s16
    from tcs_mi355.harness import InputPadder
    K_raw = torch.as_tensor(seq.K, dtype=torch.float32, device=dev)[None]
    baseline = torch.tensor([seq.baseline], dtype=torch.float32, device=dev)
    outs, state = [], None
    s16.take_flags()
    for fr in seq.frames:
        im1, im2 = D(fr.image1, dev)[None], D(fr.image2, dev)[None]
        T = D(fr.T, dev)[None]
        padder = InputPadder(im1.shape, divis_by=32)
        (im1, im2), K = padder.pad(im1, im2, K=K_raw)
        params = None if state is None else dict(K=K, T=T, previous_T=state[3], last_disp=state[0], last_net_list=state[1], fmap1=state[2],
                                                 baseline=baseline)
        o = model(im1, im2, iters=iters, test_mode=True, params=params)
        o = {"flow": o["flow"].clone(), "flow_q": o["flow_q"].clone(), "net_list": [t.clone() for t in o["net_list"]],
             "fmap1": o["fmap1"].clone()}
        outs.append(o)
        state = (o["flow_q"], o["net_list"], o["fmap1"], T)
    torch.cuda.synchronize()
    return outs, s16.take_flags()


def _equal(a, b):
    return (torch.equal(a["flow"], b["flow"]) and torch.equal(a["flow_q"], b["flow_q"]) and torch.equal(a["fmap1"], b["fmap1"])
            and all(torch.equal(x, y) for x, y in zip(a["net_list"], b["net_list"])))


def test_model_c2_clip_is_bit_reproducible(dev, det_model):
    """The 10-frame 640x480 synthetic clip at 32 iterations, free-running: two passes from graph replays and one eager pass agree bit
    for bit on every frame's flow, flow_q, net_list and fmap1 (with the float-atomic splat they differ by up to 0.15 px by frame 9,
    DESIGN.md section 7).  Domain flags stay 0."""
    from tcs_mi355 import synth
    seq = synth.make_sequence(2000, n_frames=10, height=480, width=640, max_disp=192.0)
    saved = getattr(det_model, "use_hip_graph", None)
    try:
        det_model.use_hip_graph = True
        g1, f1 = _free_run(det_model, seq, 32, dev)          # captures
        g2, f2 = _free_run(det_model, seq, 32, dev)          # replays only
        assert det_model._graphs is not None and det_model._graphs.fell_back == 0, "capture fell back to eager"
        det_model.use_hip_graph = False
        ea, fe = _free_run(det_model, seq, 32, dev)
    finally:
        det_model.use_hip_graph = saved
    assert f1 == 0 and f2 == 0 and fe == 0, (hex(f1), hex(f2), hex(fe))
    for t in range(10):
        assert _equal(g1[t], g2[t]), ("graph vs graph", t, epe(g1[t]["flow"], g2[t]["flow"]))
        assert _equal(g1[t], ea[t]), ("graph vs eager", t, epe(g1[t]["flow"], ea[t]["flow"]))
        assert all(bool(torch.isfinite(v).all()) for v in (g1[t]["flow"], g1[t]["flow_q"]))


def _prefetch_frames(dev):
    from tcs_mi355 import synth
    from tcs_mi355.harness import InputPadder
    seq = synth.make_sequence(13, n_frames=4, height=96, width=160, max_disp=32.0)
    K_raw = torch.as_tensor(seq.K, dtype=torch.float32, device=dev)[None]
    frames = []
    for fr in seq.frames:
        im1, im2 = D(fr.image1, dev)[None], D(fr.image2, dev)[None]
        padder = InputPadder(im1.shape, divis_by=32)
        (im1, im2), K = padder.pad(im1, im2, K=K_raw)
        frames.append((im1.contiguous(), im2.contiguous(), K, D(fr.T, dev)[None]))
    return frames, torch.tensor([seq.baseline], dtype=torch.float32, device=dev)


def _run_prefetch(model, frames, baseline, prefetch):
    outs, state = [], None
    for t, (i1, i2, K, T) in enumerate(frames):
        params = None if state is None else dict(K=K, T=T, previous_T=state[3], last_disp=state[0], last_net_list=state[1], fmap1=state[2],
                                                 baseline=baseline)
        o = model(i1, i2, iters=3, test_mode=True, params=params)
        if prefetch and t + 1 < len(frames):
            model.prefetch(frames[t + 1][0], frames[t + 1][1], first=False)
        state = (o["flow_q"], o["net_list"], o["fmap1"], T)
        outs.append((o["flow"].clone(), o["flow_q"].clone()))
    return outs


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_prefetch_is_bit_equal_on_temporal_frames(dev, synth_weights, det_model, precision):
    """With hip_deterministic the prefetch path equals the plain call bit for bit on EVERY frame (the float-atomic splat allows only frame
    0 to be compared so), eagerly and from graph replays, in both precision modes."""
    model = det_model if precision == "fp32" else _model(dev, synth_weights, hip_deterministic=True, hip_precision="fp16")
    frames, baseline = _prefetch_frames(dev)
    saved = getattr(model, "use_hip_graph", None)
    try:
        for graph in (True, False):
            model.use_hip_graph = graph
            plain = _run_prefetch(model, frames, baseline, False)
            n0 = model._graphs.prefetched
            piped = _run_prefetch(model, frames, baseline, True)
            assert model._graphs.prefetched - n0 == len(frames) - 1
            again = _run_prefetch(model, frames, baseline, False)
            for t in range(len(frames)):
                for k in range(2):
                    assert torch.equal(piped[t][k], plain[t][k]) and torch.equal(again[t][k], plain[t][k]), (precision, graph, t, k)
    finally:
        model.use_hip_graph = saved


def test_teacher_forced_c2_frames_vs_oracle(dev, oracle, synth_weights, det_model):
    """The first three frames of the C2 clip (640x480, 32 iterations), each temporal frame given the ORACLE's state of the previous
    frame: within the existing 1e-3 EPE bar (tests/test_gpu_parity.py::test_c2_clip_teacher_forced_vs_oracle_and_domain_flags)."""
    import os
    from tcs_mi355 import s16, synth
    from tcs_mi355.harness import InputPadder
    seq = synth.make_sequence(2000, n_frames=3, height=480, width=640, max_disp=192.0)
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    K_raw = torch.as_tensor(seq.K, dtype=torch.float32)[None]
    baseline = torch.tensor([seq.baseline], dtype=torch.float32)
    s16.take_flags()
    prev = prev_T = None
    for t, fr in enumerate(seq.frames):
        im1, im2 = torch.as_tensor(fr.image1)[None], torch.as_tensor(fr.image2)[None]
        T = torch.as_tensor(fr.T)[None]
        padder = InputPadder(im1.shape, divis_by=32)
        (im1, im2), K = padder.pad(im1, im2, K=K_raw)
        params_cpu = params_gpu = None
        if prev is not None:
            params_cpu = dict(K=K, T=T, previous_T=prev_T, last_disp=prev["flow_q"], last_net_list=prev["net_list"], fmap1=prev["fmap1"],
                              baseline=baseline)
            params_gpu = {k: ([D(x, dev) for x in v] if isinstance(v, (list, tuple)) else D(v, dev)) for k, v in params_cpu.items()}
        want = oracle.tc_stereo_forward(synth_weights, im1, im2, iters=32, params=params_cpu)
        got = det_model(D(im1, dev), D(im2, dev), iters=32, test_mode=True, params=params_gpu)
        e = epe(padder.unpad(-got["flow"]), padder.unpad(-want["flow"]))
        print(f"C2 frame {t} (deterministic, oracle state in): EPE vs oracle {e:.2e}")
        assert e <= 1e-3, (t, e)
        prev, prev_T = want, T
    assert s16.take_flags() == 0
