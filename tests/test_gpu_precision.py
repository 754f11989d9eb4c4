"""The opt-in fp16 precision mode on the MI355X: single-product contractions (tcs_conv*_desc.products = 1) against fp64 convolutions of
the fp16-ROUNDED operands, grouped launches, and the model end to end (TCStereo(args) with args.hip_precision = "fp16").

Exact semantics of one product: out = sum f16(x) * f16(w * 2^s) * 2^-s, accumulated in fp32.  f16(x) is the hi plane of the S16 split
(or of the split the fp32-tensor kernel makes), f16(w * 2^s) the hi half of the packed weight image, s its per-layer scale
(PackedConv.unscale = 2^-s).  The reference is that sum in fp64; the bound is the fp32 accumulation's:

    |got - ref| <= (K + ceil(K / 16) + 4) * 2^-24 * sum |f16(x)| |f16(w)|  +  2^-21 |ref|

K products per output, at most one rounding each plus one per 16-product MFMA step, four for the epilogue (bias, addend, activation,
scale), and 2^-21 for the S16 store (x = hi + lo).  The 3-product (fp32-grade) result is outside that bound
(test_single_product_differs_from_fp32_grade, and the 36 -> 64 1x1 shape of test_conv_f16_path_single_product): that is what makes the mode a different
arithmetic, and what a library that ignores the field fails."""
import math

import pytest
import torch
import torch.nn.functional as F

import s16_instances as si
from conftest import T, epe, maxdiff

pytestmark = pytest.mark.gpu

# end-to-end bar: tools/fp16_emulation_bar.py runs the CPU oracle with the operands of exactly the layers the mode covers
# rounded to fp16 and measures its EPE against the plain fp32 oracle: C1 (8 iterations) flow 1.99e-3, flow_q 6.7e-4; C2 frame 0 (32 iterations)
# flow 4.93e-3, flow_q 1.72e-3.  The GPU's fp16 mode differs from that emulation only in the fp32 summation order; the bar is 3x the measurement.
BAR = {"c1_flow": 3 * 1.99e-3, "c1_flow_q": 3 * 6.7e-4, "c2_flow_q": 3 * 1.72e-3}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from tcs_mi355 import native
    native.lib()
    return torch.device("cuda:0")


def D(x, dev):
    return (x if torch.is_tensor(x) else T(x)).to(dev).contiguous()


def r16(x):
    return x.float().clamp(-65504.0, 65504.0).half().double()


def rw(w, pc):
    s = round(-math.log2(pc.unscale))
    return (w.float() * 2.0 ** s).half().double() * 2.0 ** (-s)


def bound(K, S, ref):
    return (K + math.ceil(K / 16) + 4) * 2.0 ** -24 * S + 2.0 ** -21 * ref.abs()


def check(got, ref16, ref32, K, S, what):
    got = got.detach().cpu().double()
    tol = bound(K, S, ref16)
    err = (got - ref16).abs()
    assert bool((err <= tol).all()), (what, float((err / tol).max()))


CONV_CASES = [
    dict(B=1, cins=(128, 128, 128), cout=256, k=3, H=12, W=40),
    dict(B=2, cins=(32, 64, 64), cout=64, k=3, H=9, W=37),
    dict(B=1, cins=(64, 64), cout=127, k=3, H=8, W=24),
    dict(B=1, cins=(27,), cout=96, k=1, H=7, W=65),
    dict(B=1, cins=(128, 64), cout=96, k=3, H=17, W=35),
    dict(B=1, cins=(128, 64), cout=256, k=1, H=9, W=35),
    dict(B=1, cins=(64,), cout=96, k=3, H=16, W=34, stride=2),
    dict(B=1, cins=(96,), cout=128, k=3, H=15, W=33, stride=2),
    dict(B=1, cins=(64,), cout=96, k=1, H=15, W=33, stride=2),
]


@pytest.mark.parametrize("cfg", CONV_CASES)
def test_conv2d_s16_single_product(dev, cfg):
    """LINEAR on S16 sources (virtual concat, ragged grids, batch 2, stride 2 incl. the 1x1 gather): heuristic and explicit tiles."""
    from tcs_mi355 import ops, s16
    gen = torch.Generator().manual_seed(cfg["cout"] + cfg["k"] + cfg["H"])
    cin, stride, k = sum(cfg["cins"]), cfg.get("stride", 1), cfg["k"]
    w = torch.randn(cfg["cout"], cin, k, k, generator=gen) * (2.0 / (cin * k * k)) ** 0.5
    b = torch.randn(cfg["cout"], generator=gen) * 0.1
    xs = [torch.randn(cfg["B"], c, cfg["H"], cfg["W"], generator=gen) for c in cfg["cins"]]
    x = torch.cat(xs, 1)
    pc = ops.pack_conv(D(w, dev), D(b, dev), "f16x3", products=1)
    pad = k // 2
    ref16 = F.conv2d(r16(x), rw(w, pc), b.double(), padding=pad, stride=stride)
    ref32 = F.conv2d(x.double(), w.double(), b.double(), padding=pad, stride=stride)
    S = F.conv2d(r16(x).abs(), rw(w, pc).abs(), b.double().abs(), padding=pad, stride=stride)
    K = cin * k * k
    xs16 = [s16.to_s16(D(x_, dev)) for x_ in xs]
    tiles = [0] + si.linear_tiles(k, stride, cfg["cins"], cfg["cout"])       # every instance of the table (tests/s16_instances.py) for this layer
    for tc in tiles:
        _, o32 = s16.conv2d(pc, xs16, want32=True, stride=stride, tile_cfg=tc)
        check(o32, ref16, ref32, K, S, (cfg, tc))
        out = s16.zeros(cfg["B"], cfg["cout"], ref16.shape[2], ref16.shape[3], dev)
        s16.conv2d(pc, xs16, act="relu", post_scale=0.25, out16=out, stride=stride, tile_cfg=tc)
        check(out.float(), 0.25 * torch.relu(ref16), 0.25 * torch.relu(ref32), K, S, (cfg, tc, "relu"))


def test_single_product_differs_from_fp32_grade(dev):
    """disp_f_stem's shape (27 -> 96, 1x1): the 3-product result lies outside the single-product bound, the 1-product result inside it."""
    from tcs_mi355 import ops, s16
    gen = torch.Generator().manual_seed(101)
    w = torch.randn(96, 27, 1, 1, generator=gen) * (2.0 / 27) ** 0.5
    b = torch.randn(96, generator=gen) * 0.1
    x = torch.randn(1, 27, 7, 65, generator=gen)
    x16 = s16.to_s16(D(x, dev))
    p1 = ops.pack_conv(D(w, dev), D(b, dev), "f16x3", products=1)
    p3 = ops.pack_conv(D(w, dev), D(b, dev), "f16x3")
    ref16 = F.conv2d(r16(x), rw(w, p1), b.double())
    S = F.conv2d(r16(x).abs(), rw(w, p1).abs(), b.double().abs())
    tol = bound(27, S, ref16)
    one = s16.conv2d(p1, [x16], want32=True)[1].cpu().double()
    three = s16.conv2d(p3, [x16], want32=True)[1].cpu().double()
    assert bool(((one - ref16).abs() <= tol).all())
    assert bool(((three - ref16).abs() > tol).any())
    assert maxdiff(three, F.conv2d(x.double(), w.double(), b.double())) <= 2e-5


def test_out16b_and_taps_single_product(dev):
    """LINEAR with a second S16 output (out16b) and with tap partials: the K loop is single-product, the tap fold stays fp16-split."""
    from tcs_mi355 import ops, s16
    gen = torch.Generator().manual_seed(5)
    B, cin, H, W, ca, cb = 1, 64, 30, 40, 128, 64
    w = torch.randn(ca + cb, cin, 3, 3, generator=gen) * (2.0 / (cin * 9)) ** 0.5
    b = torch.randn(ca + cb, generator=gen) * 0.1
    w2 = torch.randn(2, ca, 3, 3, generator=gen) * (1.0 / (ca * 9)) ** 0.5
    x = torch.randn(B, cin, H, W, generator=gen)
    pc = ops.pack_conv(D(w, dev), D(b, dev), "f16x3", products=1)
    x16 = s16.to_s16(D(x, dev))
    ref16 = torch.relu(F.conv2d(r16(x), rw(w, pc), b.double(), padding=1))
    ref32 = torch.relu(F.conv2d(x.double(), w.double(), b.double(), padding=1))
    S = F.conv2d(r16(x).abs(), rw(w, pc).abs(), b.double().abs(), padding=1)
    oa, ob = s16.zeros(B, ca, H, W, dev), s16.zeros(B, cb, H, W, dev)
    s16.conv2d(pc, [x16], act="relu", out16=oa, out16b=ob, out16_split=ca)
    check(oa.float(), ref16[:, :ca], ref32[:, :ca], cin * 9, S[:, :ca], "out16")
    check(ob.float(), ref16[:, ca:], ref32[:, ca:], cin * 9, S[:, ca:], "out16b")
    # tap partials of a following 3x3 convolution to two channels, over the first ca channels (4 tiles)
    pca = ops.pack_conv(D(w[:ca].contiguous(), dev), D(b[:ca].contiguous(), dev), "f16x3", products=1)
    tw = s16.pack_taps(D(w2, dev))
    for tc in (1411, 1412, 1812, 21812):
        taps = s16.Taps(torch.zeros(B, 4, 18, H, W, device=dev), 4, 2, None)
        o, _ = s16.conv2d(pca, [x16], act="relu", taps=taps, tap_weights=tw, out16=s16.zeros(B, ca, H, W, dev), tile_cfg=tc)
        check(o.float(), ref16[:, :ca], ref32[:, :ca], cin * 9, S[:, :ca], ("taps out", tc))
        got = s16.taps_sum(taps)
        want = F.conv2d(o.float().cpu().double(), w2.double(), padding=1)
        assert maxdiff(got, want) <= 2e-5 * float(want.abs().max()) + 1e-6, tc


def test_gru_pair_single_product(dev):
    """GRU_ZR then GRU_Q (in-place state update) on S16 tensors, 3x3 and 1x1 cells."""
    from tcs_mi355 import ops, s16
    gen = torch.Generator().manual_seed(9)
    for k, keep_z, cx in ((3, False, (128, 128)), (1, True, (64,))):
        hid, H, W = 128, 10, 37
        cin = hid + sum(cx)
        wzr = torch.randn(2 * hid, cin, k, k, generator=gen) * (1.0 / (cin * k * k)) ** 0.5
        wq = torch.randn(hid, cin, k, k, generator=gen) * (1.0 / (cin * k * k)) ** 0.5
        bzr, bq = torch.randn(2 * hid, generator=gen) * 0.1, torch.randn(hid, generator=gen) * 0.1
        h = torch.tanh(torch.randn(1, hid, H, W, generator=gen))
        xs = [torch.randn(1, c, H, W, generator=gen) for c in cx]
        cz, cr, cq = (torch.randn(1, hid, H, W, generator=gen) * 0.3 for _ in range(3))
        pzr = ops.pack_conv(D(wzr, dev), D(bzr, dev), "f16x3", products=1)
        pq = ops.pack_conv(D(wq, dev), D(bq, dev), "f16x3", products=1)
        hx = torch.cat([h, *xs], 1)
        zr16 = F.conv2d(r16(hx), rw(wzr, pzr), bzr.double(), padding=k // 2)
        zr32 = F.conv2d(hx.double(), wzr.double(), bzr.double(), padding=k // 2)
        Szr = F.conv2d(r16(hx).abs(), rw(wzr, pzr).abs(), bzr.double().abs(), padding=k // 2)
        h16, xs16 = s16.to_s16(D(h, dev)), [s16.to_s16(D(x, dev)) for x in xs]
        zz, rh = s16.gru_gates(pzr, [h16, *xs16], h16, D(cz, dev), D(cr, dev))
        # sigmoid is 1/4-Lipschitz and |h| <= 1: the pre-activation bound carries over
        check(zz, torch.sigmoid(zr16[:, :hid] + cz), torch.sigmoid(zr32[:, :hid] + cz), cin * k * k, Szr[:, :hid], ("z", k))
        check(rh.float(), torch.sigmoid(zr16[:, hid:] + cr) * h, torch.sigmoid(zr32[:, hid:] + cr) * h, cin * k * k, Szr[:, hid:], ("rh", k))
        rhx = torch.cat([rh.float().cpu(), *xs], 1)                # the GPU's r*h: the Q launch is checked on its own inputs
        q16 = torch.tanh(F.conv2d(r16(rhx), rw(wq, pq), bq.double(), padding=k // 2) + cq)
        q32 = torch.tanh(F.conv2d(rhx.double(), wq.double(), bq.double(), padding=k // 2) + cq)
        Sq = F.conv2d(r16(rhx).abs(), rw(wq, pq).abs(), bq.double().abs(), padding=k // 2)
        z = zz.cpu().double()
        blend = (lambda q: z * h + (1 - z) * q) if keep_z else (lambda q: (1 - z) * h + z * q)
        out = s16.gru_update(pq, [rh, *xs16], h16, zz, D(cq, dev), keep_z=keep_z, out=h16)
        assert out is h16
        check(h16.float(), blend(q16), blend(q32), cin * k * k, Sq + 4 * h.abs().double(), ("h'", k))


def test_deconv_single_product_with_fused_instance_norm(dev):
    """DECONV2X with the fused InstanceNorm sums: the output against the rounded fp64 transposed convolution, the sums against the output."""
    from tcs_mi355 import ops, s16
    gen = torch.Generator().manual_seed(23)
    for cin, cout, H, W, B in ((128, 96, 30, 40, 1), (64, 32, 7, 37, 2)):
        wt = torch.randn(cin, cout, 4, 4, generator=gen) * (1.0 / (cin * 4)) ** 0.5
        x = torch.randn(B, cin, H, W, generator=gen) + 0.3
        pc = ops.pack_deconv4x4s2(D(wt, dev), products=1)
        ref16 = F.conv_transpose2d(r16(x), rw(wt, pc), stride=2, padding=1)
        ref32 = F.conv_transpose2d(x.double(), wt.double(), stride=2, padding=1)
        S = F.conv_transpose2d(r16(x).abs(), rw(wt, pc).abs(), stride=2, padding=1)
        x16 = s16.to_s16(D(x, dev))
        for tc in (0, 1412):
            ws = s16.deconv_in_stats_workspace(B, cout, H, W, dev)
            y = s16.deconv4x4s2(pc, [x16], in_stats=ws, tile_cfg=tc)
            check(y.float(), ref16, ref32, cin * 9, S, ("deconv", cout, tc))
            two = s16.instance_norm(y, act="leaky")
            got = s16.instance_norm_apply(y, ws, act="leaky")
            assert maxdiff(got.float(), two.float()) <= 2e-6, (cout, tc)


def test_blend9_single_product(dev):
    """w_head's 1x1 convolution with the softmax blend as its epilogue: logits from the single-product contraction."""
    from tcs_mi355 import ops, s16
    gen = torch.Generator().manual_seed(31)
    B, H, W = 1, 24, 40
    x = torch.randn(B, 128, H, W, generator=gen)
    w = torch.randn(9, 128, 1, 1, generator=gen) * (2.0 / 128) ** 0.5
    b = torch.randn(9, generator=gen) * 0.1
    cand = torch.randn(B, 9, H, W, generator=gen) * 4
    disp = torch.randn(B, 1, H, W, generator=gen)
    pc = ops.pack_conv(D(w, dev), D(b, dev), "f16x3", products=1)
    c1, fx = torch.empty(B, 1, H, W, device=dev), torch.empty(B, 1, H, W, device=dev)
    refined, delta = s16.conv1x1_blend(pc, [s16.to_s16(D(x, dev))], D(cand, dev), D(disp, dev), c1, fx)
    lg = F.conv2d(r16(x), rw(w, pc), b.double())
    S = F.conv2d(r16(x).abs(), rw(w, pc).abs(), b.double().abs())
    want = (torch.softmax(lg, 1) * cand.double()).sum(1, keepdim=True)
    # d(refined)/d(logit_k) = p_k (cand_k - refined): bounded by the candidates' spread
    tol = float(bound(128, S, lg).max()) * float(cand.max() - cand.min()) + 1e-5
    assert maxdiff(refined, want) <= tol
    assert maxdiff(delta, want - disp.double()) <= tol + 1e-6


def test_grouped_single_product_equals_separate(dev):
    """tcs_conv2d_s16_group with products = 1 on both sides: the loop's pairs fuse and are bit-equal to separate launches; a 1-product
    layer beside a 3-product one runs as two launches, each bit-equal to its own separate launch."""
    from tcs_mi355 import ops, s16
    gen = torch.Generator().manual_seed(11)

    def layer(cin, cout, k, H, W, products):
        x = torch.randn(1, cin, H, W, generator=gen)
        w = torch.randn(cout, cin, k, k, generator=gen) * (2.0 / (k * k * cin)) ** 0.5
        b = torch.randn(cout, generator=gen) * 0.1
        return s16.to_s16(D(x, dev)), ops.pack_conv(D(w, dev), D(b, dev), "f16x3", products=products)

    cases = [
        ((64, 64, 3, 13, 37, 1), 101412, (64, 64, 3, 13, 37, 1), 101412, True),
        ((32, 32, 3, 120, 160, 1), 0, (64, 64, 3, 120, 160, 1), 0, True),
        ((192, 96, 3, 11, 40, 1), 101812, (27, 96, 1, 11, 40, 1), 101422, True),
        ((192, 96, 3, 120, 160, 1), 101411, (27, 96, 1, 120, 160, 1), 0, True),
        ((64, 64, 3, 13, 37, 1), 101412, (64, 64, 3, 13, 37, 3), 101412, False),       # mismatched counts: two launches
        ((27, 96, 1, 11, 40, 0), 101422, (192, 96, 3, 11, 40, 1), 101812, False),
    ]
    for la, ta, lb, tb, fused in cases:
        xa16, pca = layer(*la)
        xb16, pcb = layer(*lb)
        sep_a, _ = s16.conv2d(pca, [xa16], act="relu", tile_cfg=ta)
        sep_b, _ = s16.conv2d(pcb, [xb16], act="relu", tile_cfg=tb)
        with s16.grouped(report=True) as g:
            grp_a, _ = s16.conv2d(pca, [xa16], act="relu", tile_cfg=ta)
            grp_b, _ = s16.conv2d(pcb, [xb16], act="relu", tile_cfg=tb)
        assert g.fused == [fused], (la, lb, g.fused)
        assert torch.equal(grp_a.data, sep_a.data) and torch.equal(grp_b.data, sep_b.data), (la, lb)
    # and the two product counts really are different launches: a 1-product result differs from the 3-product one
    x16, p1 = layer(64, 64, 3, 13, 37, 1)
    p3 = ops.PackedConv(p1.weight, p1.bias, p1.cout, p1.cin, p1.ksize, p1.math, p1.unscale, 0)
    assert not torch.equal(s16.conv2d(p1, [x16])[0].data, s16.conv2d(p3, [x16])[0].data)


F16_CASES = [
    # (B, cin, cout, k, H, W, stride): the plain kernel with 32- and 64-channel tiles, both wave-specialised sizes, 1x1, stride 2
    (1, 128, 128, 3, 120, 160, 1),
    (1, 64, 64, 3, 60, 80, 1),
    (1, 64, 64, 3, 20, 40, 1),
    (2, 48, 96, 3, 61, 83, 1),
    (1, 36, 64, 1, 60, 80, 1),
    (1, 96, 128, 1, 30, 40, 1),
    (1, 64, 96, 3, 61, 83, 2),
]


@pytest.mark.parametrize("case", F16_CASES)
def test_conv_f16_path_single_product(dev, case):
    """tcs_conv2d (fp32 NCHW tensors, k_conv_f16x1 / k_conv_f16x1_ws): the split the kernel makes is rounded the same way."""
    from tcs_mi355 import ops
    B, cin, cout, k, H, W, stride = case
    gen = torch.Generator().manual_seed(cin + cout + H)
    w = torch.randn(cout, cin, k, k, generator=gen) * (2.0 / (cin * k * k)) ** 0.5
    b = torch.randn(cout, generator=gen) * 0.1
    x = torch.randn(B, cin, H, W, generator=gen)
    pc = ops.pack_conv(D(w, dev), D(b, dev), "f16x3", products=1)
    got = ops.conv2d(pc, [D(x, dev)], act="relu", stride=stride)
    pad = k // 2
    ref16 = torch.relu(F.conv2d(r16(x), rw(w, pc), b.double(), padding=pad, stride=stride))
    ref32 = torch.relu(F.conv2d(x.double(), w.double(), b.double(), padding=pad, stride=stride))
    S = F.conv2d(r16(x).abs(), rw(w, pc).abs(), b.double().abs(), padding=pad, stride=stride)
    check(got, ref16, ref32, cin * k * k, S, case)
    if cin * k * k <= 64:            # (for long sums the worst-case accumulation bound also covers the rounding of the operands)
        assert bool(((ref32 - ref16).abs() > bound(cin * k * k, S, ref16)).any()), case


def test_conv_f16_path_deconv_and_gru_single_product(dev):
    """The fp32-tensor transposed convolution and GRU epilogues on the single-product kernel."""
    from tcs_mi355 import ops
    gen = torch.Generator().manual_seed(3)
    cin, cout, H, W = 96, 64, 15, 20
    wt = torch.randn(cin, cout, 4, 4, generator=gen) * (1.0 / (cin * 4)) ** 0.5
    x = torch.randn(1, cin, H, W, generator=gen)
    pc = ops.pack_deconv4x4s2(D(wt, dev), products=1)
    got = ops.deconv4x4s2(pc, [D(x, dev)])
    ref16 = F.conv_transpose2d(r16(x), rw(wt, pc), stride=2, padding=1)
    ref32 = F.conv_transpose2d(x.double(), wt.double(), stride=2, padding=1)
    check(got, ref16, ref32, cin * 9, F.conv_transpose2d(r16(x).abs(), rw(wt, pc).abs(), stride=2, padding=1), "deconv")
    hid, cx = 64, 64
    wzr = torch.randn(2 * hid, hid + cx, 3, 3, generator=gen) * (1.0 / ((hid + cx) * 9)) ** 0.5
    bzr = torch.randn(2 * hid, generator=gen) * 0.1
    h = torch.tanh(torch.randn(1, hid, H, W, generator=gen))
    xx = torch.randn(1, cx, H, W, generator=gen)
    pzr = ops.pack_conv(D(wzr, dev), D(bzr, dev), "f16x3", products=1)
    z, rh = ops.gru_gates(pzr, [D(h, dev), D(xx, dev)], D(h, dev))
    hx = torch.cat([h, xx], 1)
    zr16 = F.conv2d(r16(hx), rw(wzr, pzr), bzr.double(), padding=1)
    zr32 = F.conv2d(hx.double(), wzr.double(), bzr.double(), padding=1)
    S = F.conv2d(r16(hx).abs(), rw(wzr, pzr).abs(), bzr.double().abs(), padding=1)
    check(z, torch.sigmoid(zr16[:, :hid]), torch.sigmoid(zr32[:, :hid]), (hid + cx) * 9, S[:, :hid], "z")
    check(rh, torch.sigmoid(zr16[:, hid:]) * h, torch.sigmoid(zr32[:, hid:]) * h, (hid + cx) * 9, S[:, hid:], "rh")


# ------------------------------------------------------------------------------------------------
# end to end
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
def models(dev, synth_weights):
    return {"default": _model(dev, synth_weights), "fp32": _model(dev, synth_weights, hip_precision="fp32"),
            "fp16": _model(dev, synth_weights, hip_precision="fp16")}


def _c1(dev):
    from tcs_mi355 import synth
    from tcs_mi355.harness import InputPadder
    pr = synth.make_pair(1)
    i1, i2 = D(pr.image1, dev)[None], D(pr.image2, dev)[None]
    return InputPadder(i1.shape, divis_by=32).pad(i1, i2)


def test_e2e_fp32_mode_is_the_default_bit_for_bit(dev, models):
    """hip_precision="fp32" is today's behaviour: frame 0 is bit-reproducible, so bit-equal to a model built without it."""
    p1, p2 = _c1(dev)
    a = models["default"](p1, p2, iters=8, test_mode=True)
    b = models["fp32"](p1, p2, iters=8, test_mode=True)
    for k in ("flow", "flow_q", "fmap1"):
        assert torch.equal(a[k], b[k]), k


def test_e2e_fp16_c1_within_bar(dev, models, e2e_golden):
    """C1 (320x240 padded to 320x256, 8 iterations): fp16 differs from fp32 and stays within the measured bar of the fp32 reference."""
    from tcs_mi355 import s16
    p1, p2 = _c1(dev)
    s16.take_flags()
    out16 = models["fp16"](p1, p2, iters=8, test_mode=True)
    assert s16.take_flags() == 0
    out32 = models["fp32"](p1, p2, iters=8, test_mode=True)
    assert not torch.equal(out16["flow"], out32["flow"])
    for k in ("flow", "flow_q", "fmap1"):
        assert bool(torch.isfinite(out16[k]).all()), k
    assert epe(out16["flow"], e2e_golden["c1_flow"]) <= BAR["c1_flow"]
    assert epe(out16["flow_q"], e2e_golden["c1_flow_q"]) <= BAR["c1_flow_q"]


def test_e2e_fp16_c2_frame0_within_bar(dev, models, e2e_golden):
    """C2 frame 0 (640x480, 32 iterations) against the reference's output."""
    from tcs_mi355 import s16, synth
    fr = synth.make_sequence(2000, n_frames=1).frames[0]
    s16.take_flags()
    out = models["fp16"](D(fr.image1, dev)[None], D(fr.image2, dev)[None], iters=32, test_mode=True)
    assert s16.take_flags() == 0
    assert bool(torch.isfinite(out["flow_q"]).all())
    assert epe(out["flow_q"], e2e_golden["c2_flow_q"]) <= BAR["c2_flow_q"]


def test_e2e_fp16_graph_replay_matches_eager(dev, models):
    """The fp16 model runs captured and eager.  Frame 0 (no splat atomics) is bit-equal, which is what shows that the captured graph runs
    the same single-product kernels.  Temporal frames get a wider tolerance than test_gpu_parity.py::test_graph_replay_matches_eager's 1e-5:
    the splat's float atomics make them differ from run to run (~1e-6 px in the fp32 mode), and fp16 operands turn that into rounding
    flips of 2^-11.  Measured on MI355X, fp16 mode, this clip: eager against eager 2.8e-4 / 4.4e-4 px on frames 1 / 2, graph against eager
    2.8e-4 .. 4.0e-4 / 4.4e-4 .. 4.6e-4.  Bar: 2e-3."""
    from tcs_mi355 import synth
    from tcs_mi355.harness import run_sequence
    model = models["fp16"]
    seq = synth.make_sequence(11, n_frames=3, height=96, width=128, max_disp=32.0)
    model.use_hip_graph = False
    eager = []
    run_sequence(model, seq, iters=3, device=dev, collect=eager)
    model.use_hip_graph = True
    graphed, again = [], []
    run_sequence(model, seq, iters=3, device=dev, collect=graphed)
    run_sequence(model, seq, iters=3, device=dev, collect=again)
    assert model._graphs is not None and model._graphs.fell_back == 0, "capture fell back to eager"
    assert torch.equal(graphed[0], eager[0]) and torch.equal(again[0], eager[0])
    for t in (1, 2):
        assert epe(graphed[t], eager[t]) <= 2e-3 and epe(again[t], eager[t]) <= 2e-3, t
