"""Every tile instance of tcs_conv2d_s16 (csrc/tcs_conv_s16.hip) against fp64 PyTorch on the CPU, per epilogue and tile.

The cases are parametrised from tests/s16_instances.py — the table that test_s16_instances_host.py proves equal to the library's
own switch — times `products` (3: the fp16-split contraction, 1: fp16 operands).  A table row the library refuses is a failure.
Every instance runs on a RAGGED grid (13 x 70, batch 3: interior, last-column and last-row patches for 4-, 5- and 8-row tiles;
several virtual sources, the last one not a multiple of 16 channels; for the 1x1 tiles with 2 / 4 k-steps per stage a last source
whose k-steps are padded up to the stage size); the loop's layers also run at their real shapes with the heuristic's tile, and the
last test runs the model with a recorder in front of the launch and asserts that it launches nothing this module did not cover.

Beyond the values, every case asserts: the S16 outputs' border rows / columns, padding channels and spare groups are exactly zero
and a foreign channel of a shared 8-group keeps its bits; every fp32 output is a view into a larger sentinel-filled buffer whose
surroundings stay untouched and whose inside is fully written; the domain flags stay clear.

Bars (the project's own, tests/test_gpu_s16.py and tests/test_gpu_precision.py): three products — LINEAR / stride 2 / DECONV2X <= 2e-5
with fan-in-scaled weights, GRU outputs <= 1e-5, tap sums <= 3e-5, BLEND9 <= 2e-4 on `refined` with candidates below 50; one product —
the fp32-accumulation bound of test_gpu_precision.py (`check` / `bound` on the fp16-rounded operands)."""
import contextlib
import math

import pytest
import torch
import torch.nn.functional as F

import s16_instances as si
from conftest import maxdiff
from test_gpu_precision import bound, check, r16, rw

pytestmark = pytest.mark.gpu

SENT = -1.5e38                  # sentinel of the fp32 guard buffers: no output of these cases comes near it
PAD = 4096                      # guard elements on each side of an fp32 output (more than a row of the widest grid)
RH, RW, RB = 13, 70, 3          # the ragged grid: 13 % 4, 13 % 5, 13 % 8, 13 % 10, 13 % 16 != 0; 70 = 2 * 32 + 6
LIN_CINS = {1: (32, 16, 27), 2: (32, 40), 4: (64, 91)}     # by k-steps per stage: (.., 40) pads 3 -> 4 k-steps, (.., 91) 6 -> 8
GRU_XS = {1: (16, 27), 2: (40,), 4: (91,)}                  # beside the 64-channel hidden state (4 k-steps)
HID = 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from tcs_mi355 import native
    native.lib()
    return torch.device("cuda:0")


def D(x, dev):
    return x.float().to(dev).contiguous()


class Guard:
    """An fp32 output as a view into a larger buffer filled with a sentinel."""

    def __init__(self, shape, dev):
        self.n = math.prod(shape)
        self.buf = torch.full((self.n + 2 * PAD,), SENT, dtype=torch.float32, device=dev)
        self.view = self.buf[PAD:PAD + self.n].view(*shape)

    def check(self, what):
        b = self.buf.cpu()
        assert bool((b[:PAD] == SENT).all()), (what, "written before the output")
        assert bool((b[PAD + self.n:] == SENT).all()), (what, "written behind the output")
        assert not bool((b[PAD:PAD + self.n] == SENT).any()), (what, "elements of the output left unwritten")


def channels(t):
    """fp16 [B, G*8, 2, H+2, W+2] view of an S16 tensor's storage."""
    d = t.data
    return d.permute(0, 1, 5, 2, 3, 4).reshape(d.shape[0], d.shape[1] * 8, 2, d.shape[3], d.shape[4])


def s16_clean(t, c_real, what, c_from=0):
    """Border rows / columns of every group, and every channel outside [c_from, c_real), are exactly zero."""
    d = t.data
    assert int(torch.count_nonzero(d[:, :, :, 0])) == 0 and int(torch.count_nonzero(d[:, :, :, -1])) == 0, (what, "border row")
    assert int(torch.count_nonzero(d[:, :, :, :, 0])) == 0 and int(torch.count_nonzero(d[:, :, :, :, -1])) == 0, (what, "border column")
    ch = channels(t)
    assert int(torch.count_nonzero(ch[:, c_real:])) == 0 and int(torch.count_nonzero(ch[:, :c_from])) == 0, (what, "padding channels")


def sources(s16, gen, B, cins, H, W, dev, kst=1, scale=1.0):
    """CPU tensors and their S16 images; the last source is allocated with the groups that `kst` k-steps per stage need."""
    xs = [torch.randn(B, c, H, W, generator=gen) * scale for c in cins]
    out = []
    for i, x in enumerate(xs):
        k = (x.shape[1] + 15) // 16
        g = 2 * (-(-k // kst) * kst) if i + 1 == len(xs) else 2 * k
        out.append(s16.to_s16(D(x, dev), out=s16.zeros(B, x.shape[1], H, W, dev, groups=g)))
    return xs, out


@contextlib.contextmanager
def planned(monkeypatch, log):
    """Record the instance tcs_conv2d_s16_plan names for every tcs_conv2d_s16 launch made inside the block (then launch it)."""
    from tcs_mi355 import native, s16
    fwd = s16._launch

    def recorder(d, name, keep):
        rc, p = si.plan(native, native.lib(), d)
        assert rc == si.TCS_OK, (name, rc)
        log.append(si.instance_key(p))
        return fwd(d, name, keep)

    with monkeypatch.context() as m:
        m.setattr(s16, "_launch", recorder)
        yield


def expect_instance(log, inst, products):
    k, s, e, t, code = inst
    want = (k, s, e, t, products) + si.digits(code)
    assert log and all(v == want for v in log), (si.inst_id(inst), want, sorted(set(log)))


class Close:
    """The bar of one product count: 3 -> absolute `bar` against fp64 of the operands; 1 -> test_gpu_precision.check on the rounded ones."""

    def __init__(self, products, pc=None):
        self.p, self.pc = products, pc

    def x(self, t):
        return r16(t) if self.p == 1 else t.double()

    def w(self, t):
        return rw(t, self.pc) if self.p == 1 else t.double()

    def __call__(self, got, ref, bar, K, S, what):
        if self.p == 1:
            check(got, ref, None, K, S, what)
        else:
            e = maxdiff(got, ref)
            assert e <= bar, (what, e)


# ---------------------------------------------------------------------------------------------------------------------
# per-epilogue runners (shared by the ragged and the real-shape cases)
# ---------------------------------------------------------------------------------------------------------------------
def run_linear(dev, ksize, stride, cins, cout, B, H, W, products, tile_cfg, kst=1, variants=True, cpu32=False):
    from tcs_mi355 import ops, s16
    gen = torch.Generator().manual_seed(1000 * ksize + 100 * stride + cout + H)
    cin, pad = sum(cins), ksize // 2
    w = torch.randn(cout, cin, ksize, ksize, generator=gen) * (2.0 / (cin * ksize * ksize)) ** 0.5
    b = torch.randn(cout, generator=gen) * 0.1
    xs, xs16 = sources(s16, gen, B, cins, H, W, dev, kst)
    x = torch.cat(xs, 1)
    pc = ops.pack_conv(D(w, dev), D(b, dev), "f16x3", products=products)
    c = Close(products, pc)
    ref = F.conv2d(c.x(x), c.w(w), b.double(), padding=pad, stride=stride)
    S = F.conv2d(c.x(x).abs(), c.w(w).abs(), b.double().abs(), padding=pad, stride=stride) if products == 1 else None
    K, (Ho, Wo) = cin * ksize * ksize, ref.shape[2:]
    if cpu32 and products == 3:     # the fp32 CPU convolution of the same inputs is inside the bar: a failure below is the kernel's
        assert maxdiff(F.conv2d(x, w, b, padding=pad, stride=stride), F.conv2d(x.double(), w.double(), b.double(), padding=pad, stride=stride)) <= 2e-5
    cpad = (cout + 15) // 16 * 16
    what = (ksize, stride, cout, tile_cfg, products)

    def out_buffer():
        # a buffer with spare groups; when Cout leaves part of an 8-group free (127 of 128), that channel belongs to someone else
        o = s16.zeros(B, cpad, Ho, Wo, dev, groups=cpad // 8 + 2)
        foreign = None
        if cout % 8:
            foreign = torch.randn(B, 1, Ho, Wo, generator=gen) * 20
            for ch in range(cout, (cout + 7) // 8 * 8):
                s16.set_channel(D(foreign, dev), o, ch)
        return o, (channels(o)[:, cout:(cout + 7) // 8 * 8].clone() if foreign is not None else None)

    def out_check(o, before, tag):
        hi = (cout + 7) // 8 * 8
        if before is not None:
            assert torch.equal(channels(o)[:, cout:hi], before), (what, tag, "foreign channel changed")
        d = o.data
        assert int(torch.count_nonzero(d[:, :, :, 0])) == 0 and int(torch.count_nonzero(d[:, :, :, -1])) == 0, (what, tag, "border row")
        assert int(torch.count_nonzero(d[:, :, :, :, 0])) == 0 and int(torch.count_nonzero(d[:, :, :, :, -1])) == 0, (what, tag, "border column")
        assert int(torch.count_nonzero(channels(o)[:, hi:])) == 0, (what, tag, "padding channels")

    # (a) out16 and out32 of one launch
    o, before = out_buffer()
    g32 = Guard((B, cout, Ho, Wo), dev)
    s16.conv2d(pc, xs16, out16=o, out32=g32.view, stride=stride, tile_cfg=tile_cfg)
    g32.check((what, "out32"))
    out_check(o, before, "plain")
    c(g32.view, ref, 2e-5, K, S, (what, "out32"))
    c(s16.from_s16(o, cout), ref, 2e-5, K, S, (what, "out16"))
    if not variants:
        return
    # (b) relu + fp32 addend + post_scale
    add = torch.randn(B, cout, Ho, Wo, generator=gen)
    o, before = out_buffer()
    s16.conv2d(pc, xs16, act="relu", addend=D(add, dev), post_scale=0.25, out16=o, stride=stride, tile_cfg=tile_cfg)
    out_check(o, before, "relu+addend")
    c(s16.from_s16(o, cout), 0.25 * torch.relu(ref + add.double()), 2e-5, K, None if S is None else S + add.abs().double(), (what, "relu+addend"))
    # (c) the tail of a residual block: relu(relu(v) + skip) with an S16 skip
    skip = torch.randn(B, cout, Ho, Wo, generator=gen)
    o, before = out_buffer()
    s16.conv2d(pc, xs16, act="relu_add_relu", addend16=s16.to_s16(D(skip, dev)), out16=o, stride=stride, tile_cfg=tile_cfg)
    out_check(o, before, "relu_add_relu")
    c(s16.from_s16(o, cout), torch.relu(torch.relu(ref) + skip.double()), 2e-5, K, None if S is None else S + skip.abs().double(), (what, "relu_add_relu"))


def run_taps(dev, cins, B, H, W, products, tile_cfg):
    """conv1 (-> 64 channels folded into the tap partials of a 3x3 conv2 to 2 channels, + 40 channels to out16b)."""
    from tcs_mi355 import ops, s16
    gen = torch.Generator().manual_seed(77 + H)
    cin, cmid, extra, nout = sum(cins), 64, 40, 2
    w1 = torch.randn(cmid + extra, cin, 3, 3, generator=gen) * (2.0 / (9 * cin)) ** 0.5
    b1 = torch.randn(cmid + extra, generator=gen) * 0.1
    w2 = torch.randn(nout, cmid, 3, 3, generator=gen) * (2.0 / (9 * cmid)) ** 0.5
    b2 = torch.randn(nout, generator=gen) * 0.1
    xs, xs16 = sources(s16, gen, B, cins, H, W, dev)
    x = torch.cat(xs, 1)
    pc = ops.pack_conv(D(w1, dev), D(b1, dev), "f16x3", products=products)
    c = Close(products, pc)
    y = torch.relu(F.conv2d(c.x(x), c.w(w1), b1.double(), padding=1))
    S = F.conv2d(c.x(x).abs(), c.w(w1).abs(), b1.double().abs(), padding=1) if products == 1 else None
    ntile = cmid // 32
    g = Guard((B, ntile, 9 * nout, H, W), dev)
    taps = s16.Taps(g.view, ntile, nout, D(b2, dev))
    first = s16.zeros(B, cmid, H, W, dev, groups=cmid // 8 + 2)
    second = s16.zeros(B, extra, H, W, dev, groups=(extra + 15) // 16 * 2 + 2)
    what = ("taps", tile_cfg, products)
    s16.conv2d(pc, xs16, act="relu", taps=taps, tap_weights=s16.pack_taps(D(w2, dev)), out16=first, out16b=second, out16_split=cmid,
               tile_cfg=tile_cfg)
    g.check(what)
    s16_clean(first, cmid, (what, "out16"))
    s16_clean(second, extra, (what, "out16b"))
    c(s16.from_s16(first, cmid), y[:, :cmid], 2e-5, cin * 9, None if S is None else S[:, :cmid], (what, "out16"))
    c(s16.from_s16(second, extra), y[:, cmid:], 2e-5, cin * 9, None if S is None else S[:, cmid:], (what, "out16b"))
    got = s16.taps_sum(taps)
    if products == 3:
        e = maxdiff(got, F.conv2d(y[:, :cmid], w2.double(), b2.double(), padding=1))
        assert e <= 3e-5, (what, e)
    else:       # the fold stays an fp16-split contraction: against the GPU's own (single-product) first layer
        want = F.conv2d(s16.from_s16(first, cmid).cpu().double(), w2.double(), b2.double(), padding=1)
        assert maxdiff(got, want) <= 2e-5 * float(want.abs().max()) + 1e-6, what


def run_gru_zr(dev, ksize, xcs, hid, B, H, W, products, tile_cfg, kst=1, cpu32=False):
    from tcs_mi355 import ops, s16
    gen = torch.Generator().manual_seed(9 + ksize + H)
    cin, pad = hid + sum(xcs), ksize // 2
    wzr = torch.randn(2 * hid, cin, ksize, ksize, generator=gen) * (1.0 / (cin * ksize * ksize)) ** 0.5
    bzr = torch.randn(2 * hid, generator=gen) * 0.1
    h = torch.tanh(torch.randn(B, hid, H, W, generator=gen))
    xs, xs16 = sources(s16, gen, B, xcs, H, W, dev, kst)
    ctx = torch.randn(B, 2 * hid, H, W, generator=gen) * 0.3
    hx = torch.cat([h, *xs], 1)
    pzr = ops.pack_conv(D(wzr, dev), D(bzr, dev), "f16x3", products=products)
    c = Close(products, pzr)
    pre = F.conv2d(c.x(hx), c.w(wzr), bzr.double(), padding=pad) + ctx.double()
    S = F.conv2d(c.x(hx).abs(), c.w(wzr).abs(), bzr.double().abs(), padding=pad) + ctx.abs().double() if products == 1 else None
    z_ref, rh_ref = torch.sigmoid(pre[:, :hid]), torch.sigmoid(pre[:, hid:]) * h.double()
    if cpu32 and products == 3:     # the fp32 CPU convolution is inside the bars; for K = 3456 the relative bar of test_f16x3_split_is_fp32_grade
        p32 = F.conv2d(hx, wzr, bzr, padding=pad) + ctx
        assert maxdiff(torch.sigmoid(p32), torch.sigmoid(pre)) <= 1e-5 and maxdiff(p32, pre) / float(pre.abs().max()) <= 1e-5
    h16 = s16.to_s16(D(h, dev))
    ctx_d = D(ctx, dev)
    K = cin * ksize * ksize
    for sliced in (False, True):
        what = ("gru_zr", ksize, tile_cfg, products, "sliced" if sliced else "plain")
        gz = Guard((B, hid, H, W), dev)
        rh = s16.zeros(B, hid, H, W, dev, groups=hid // 8 + 2)
        if sliced:
            s16.gru_gates(pzr, [h16, *xs16], h16, ctx_d[:, :hid], ctx_d[:, hid:], z_out=gz.view, rh_out=rh, tile_cfg=tile_cfg, addend_ctot=2 * hid)
        else:
            s16.gru_gates(pzr, [h16, *xs16], h16, ctx_d[:, :hid].contiguous(), ctx_d[:, hid:].contiguous(), z_out=gz.view, rh_out=rh,
                          tile_cfg=tile_cfg)
        gz.check(what)
        s16_clean(rh, hid, what)
        c(gz.view, z_ref, 1e-5, K, None if S is None else S[:, :hid], (what, "z"))
        c(s16.from_s16(rh, hid), rh_ref, 1e-5, K, None if S is None else S[:, hid:], (what, "rh"))


def run_gru_q(dev, ksize, xcs, hid, B, H, W, products, tile_cfg, kst=1, cpu32=False):
    """The Q launch on its own: fed the reference's z and r * h."""
    from tcs_mi355 import ops, s16
    gen = torch.Generator().manual_seed(19 + ksize + H)
    cin, pad = hid + sum(xcs), ksize // 2
    wq = torch.randn(hid, cin, ksize, ksize, generator=gen) * (1.0 / (cin * ksize * ksize)) ** 0.5
    bq = torch.randn(hid, generator=gen) * 0.1
    h = torch.tanh(torch.randn(B, hid, H, W, generator=gen))
    z = torch.sigmoid(torch.randn(B, hid, H, W, generator=gen))
    rh = torch.sigmoid(torch.randn(B, hid, H, W, generator=gen)) * h
    xs, xs16 = sources(s16, gen, B, xcs, H, W, dev, kst)
    cq = torch.randn(B, hid, H, W, generator=gen) * 0.3
    rhx = torch.cat([rh, *xs], 1)
    pq = ops.pack_conv(D(wq, dev), D(bq, dev), "f16x3", products=products)
    c = Close(products, pq)
    pre = F.conv2d(c.x(rhx), c.w(wq), bq.double(), padding=pad) + cq.double()
    q = torch.tanh(pre)
    S = (F.conv2d(c.x(rhx).abs(), c.w(wq).abs(), bq.double().abs(), padding=pad) + cq.abs().double() + 4 * h.abs().double()) if products == 1 else None
    if cpu32 and products == 3:
        p32 = F.conv2d(rhx, wq, bq, padding=pad) + cq
        assert maxdiff(torch.tanh(p32), q) <= 1e-5 and maxdiff(p32, pre) / float(pre.abs().max()) <= 1e-5
    zd, hd = z.double(), h.double()
    rh16, z_d, cq_d = s16.to_s16(D(rh, dev)), D(z, dev), D(cq, dev)
    K = cin * ksize * ksize
    for keep_z, inplace in ((False, True), (True, False)):
        what = ("gru_q", ksize, tile_cfg, products, keep_z, "in place" if inplace else "out of place")
        ref = zd * hd + (1 - zd) * q if keep_z else (1 - zd) * hd + zd * q
        h16 = s16.to_s16(D(h, dev), out=s16.zeros(B, hid, H, W, dev, groups=hid // 8 + 2))
        if inplace:
            out = s16.gru_update(pq, [rh16, *xs16], h16, z_d, cq_d, keep_z=keep_z, out=h16, tile_cfg=tile_cfg)
            assert out is h16
        else:
            g = Guard((B, hid, H, W), dev)
            out = s16.zeros(B, hid, H, W, dev, groups=hid // 8 + 2)
            s16.gru_update(pq, [rh16, *xs16], h16, z_d, cq_d, keep_z=keep_z, out=out, out32=g.view, tile_cfg=tile_cfg)
            g.check(what)
            c(g.view, ref, 1e-5, K, S, (what, "out32"))
            assert maxdiff(s16.from_s16(h16, hid), h) <= 2.0 ** -21, (what, "h changed")
        s16_clean(out, hid, what)
        c(s16.from_s16(out, hid), ref, 1e-5, K, S, (what, "h'"))


def run_deconv(dev, cins, cout, B, H, W, products, tile_cfg, stats=True, cpu32=False):
    from tcs_mi355 import ops, s16
    gen = torch.Generator().manual_seed(11 + cout + H)
    cin = sum(cins)
    wt = torch.randn(cin, cout, 4, 4, generator=gen) * (1.0 / (cin * 4)) ** 0.5
    xs, xs16 = sources(s16, gen, B, cins, H, W, dev)
    x = torch.cat(xs, 1)
    pc = ops.pack_deconv4x4s2(D(wt, dev), products=products)
    c = Close(products, pc)
    ref = F.conv_transpose2d(c.x(x), c.w(wt), stride=2, padding=1)
    S = F.conv_transpose2d(c.x(x).abs(), c.w(wt).abs(), stride=2, padding=1) if products == 1 else None
    if cpu32 and products == 3:
        assert maxdiff(F.conv_transpose2d(x, wt, stride=2, padding=1), F.conv_transpose2d(x.double(), wt.double(), stride=2, padding=1)) <= 2e-5
    what = ("deconv", cout, tile_cfg, products)
    ws = s16.deconv_in_stats_workspace(B, cout, H, W, dev) if stats else None
    y = s16.zeros(B, cout, 2 * H, 2 * W, dev, groups=(cout + 15) // 16 * 2 + 2)
    s16.deconv4x4s2(pc, xs16, out16=y, in_stats=ws, tile_cfg=tile_cfg)
    s16_clean(y, cout, what)
    c(s16.from_s16(y, cout), ref, 2e-5, cin * 9, S, what)
    if stats:       # the sums against fp64 sums of the GPU's own output (bars of test_deconv_fused_instance_norm_statistics)
        ys, sums, n = s16.from_s16(y, cout).cpu().double(), ws.cpu().double(), 4.0 * H * W
        assert maxdiff(sums[..., 0] / 2 ** 20 / n, ys.mean((2, 3))) <= 2e-6, what
        assert float(((sums[..., 1] / 2 ** 16 / n - (ys * ys).mean((2, 3))).abs() / (ys * ys).mean((2, 3))).max()) <= 1e-6, what


def run_blend(dev, cins, B, H, W, products, tile_cfg, kst=1):
    from tcs_mi355 import ops, s16
    gen = torch.Generator().manual_seed(31 + H)
    cin = sum(cins)
    w = torch.randn(9, cin, 1, 1, generator=gen) * (1.0 / cin) ** 0.5
    b = torch.randn(9, generator=gen) * 0.1
    xs, xs16 = sources(s16, gen, B, cins, H, W, dev, kst)
    x = torch.cat(xs, 1)
    cand = torch.rand(B, 9, H, W, generator=gen) * 49
    disp = torch.rand(B, 1, H, W, generator=gen) * 49
    pc = ops.pack_conv(D(w, dev), D(b, dev), "f16x3", products=products)
    c = Close(products, pc)
    lg = F.conv2d(c.x(x), c.w(w), b.double())
    want = (torch.softmax(lg, 1) * cand.double()).sum(1, keepdim=True)
    if products == 3:
        bar = 2e-4
    else:       # d(refined) / d(logit_k) = p_k (cand_k - refined): bounded by the candidates' spread (test_blend9_single_product)
        S = F.conv2d(c.x(x).abs(), c.w(w).abs(), b.double().abs())
        bar = float(bound(cin, S, lg).max()) * float(cand.max() - cand.min()) + 1e-5
    what = ("blend9", tile_cfg, products)
    gs = [Guard((B, 1, H, W), dev) for _ in range(4)]
    buf = s16.zeros(B, 128, H, W, dev)
    s16.conv1x1_blend(pc, xs16, D(cand, dev), D(disp, dev), gs[2].view, gs[3].view, flow_x_s16=buf, flow_x_channel=127, refined=gs[0].view,
                      delta=gs[1].view, tile_cfg=tile_cfg)
    for g, n in zip(gs, ("refined", "delta", "coords1", "flow_x")):
        g.check((what, n))
    px = torch.arange(W, dtype=torch.float64).view(1, 1, 1, W)
    rnd = 2.0 ** -22 * (W + 50)                # one fp32 rounding of a value below W + 50 per derived plane
    assert maxdiff(gs[0].view, want) <= bar, (what, maxdiff(gs[0].view, want))
    assert maxdiff(gs[1].view, want - disp.double()) <= bar + rnd, what
    assert maxdiff(gs[2].view, px - want) <= bar + rnd, what
    assert maxdiff(gs[3].view, -want.expand(B, 1, H, W)) <= bar + 2 * rnd, what
    s16_clean(buf, 128, what, c_from=127)
    assert maxdiff(s16.from_s16(buf, 128)[:, 127:], gs[3].view) <= 2.0 ** -21 * 64, what


# ---------------------------------------------------------------------------------------------------------------------
# every instance of the table on the ragged grid
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("products", si.PRODUCTS)
@pytest.mark.parametrize("inst", si.all_instances(), ids=si.inst_id)
def test_instance_vs_fp64(dev, monkeypatch, inst, products):
    from tcs_mi355 import s16
    ksize, stride, epi, taps, code = inst
    rs, rpw, mt, rows, kst, nst = si.digits(code)
    assert RH % rows and RH % (2 * rows) and RW % 32 and RW > 32
    s16.take_flags()
    log = []
    with planned(monkeypatch, log):
        for tile_cfg in (code, 100000 + code):              # both block -> XCD mappings
            if epi == si.EPI_LINEAR and taps:
                run_taps(dev, LIN_CINS[1], RB, RH, RW, products, tile_cfg)
            elif epi == si.EPI_LINEAR:
                full = tile_cfg == code                      # the addend variants once; the second mapping repeats the plain launch
                for (H, W) in (((2 * RH + 1, 2 * RW - 1), (2 * RH, 2 * RW)) if stride == 2 else ((RH, RW),)):   # stride 2: odd and even inputs
                    for cout in ((127, 9) if mt == 1 else (128,)):
                        run_linear(dev, ksize, stride, LIN_CINS[kst], cout, RB, H, W, products, tile_cfg, kst, variants=full)
            elif epi == si.EPI_GRU_ZR:
                run_gru_zr(dev, ksize, GRU_XS[kst], HID, RB, RH, RW, products, tile_cfg, kst)
            elif epi == si.EPI_GRU_Q:
                run_gru_q(dev, ksize, GRU_XS[kst], HID, RB, RH, RW, products, tile_cfg, kst)
            elif epi == si.EPI_DECONV2X:
                run_deconv(dev, LIN_CINS[1], 32, RB, RH, RW, products, tile_cfg, stats=True)
                if mt == 1:                                  # 24 outputs per parity: 96 channels = 3 tiles, no statistics
                    run_deconv(dev, LIN_CINS[1], 24, RB, RH, RW, products, tile_cfg, stats=False)
            else:
                run_blend(dev, LIN_CINS[kst], RB, RH, RW, products, tile_cfg, kst)
    expect_instance(log, inst, products)
    assert s16.take_flags() == 0


# ---------------------------------------------------------------------------------------------------------------------
# the loop's layers at their real shapes, with the heuristic's tile
# ---------------------------------------------------------------------------------------------------------------------
def _real_cases():
    out = []
    for layer in si.LOOP_LAYERS:
        name, div = layer[0], layer[7]
        out.append((layer, si.IMAGES[0], 1, 3))
        out.append((layer, si.IMAGES[0], 1, 1))
        if div == 4:
            out.append((layer, si.IMAGES[1], 1, 3))          # the KITTI shape: 96 x 312
        if name in ("gru08.zr", "gru08.q"):
            out.append((layer, si.IMAGES[0], 4, 3))
    return out


@pytest.mark.parametrize("case", _real_cases(), ids=lambda c: f"{c[0][0]}-{c[1][1]}x{c[1][0]}-b{c[2]}-p{c[3]}")
def test_loop_layer_real_shape(dev, monkeypatch, case):
    """tile_cfg = 0 at the size the model runs the layer: the launch is the instance the planner names for the layer (the host test's
    list), that instance is a row of the table, and the result meets the same bars (K = 3456 for gru08)."""
    from tcs_mi355 import native, s16
    (name, ksize, stride, epi, taps, cins, cout, div), image, B, products = case
    H, W = si.layer_grid(image, div)
    rc, p = si.plan(native, native.lib(), si.host_desc(native, ksize, stride, epi, taps, cins, cout, H, W, B=B, products=products))
    assert rc == si.TCS_OK and si.instance_key(p) in si.table_keys(), (name, rc)
    s16.take_flags()
    log = []
    with planned(monkeypatch, log):
        if epi == si.EPI_LINEAR:
            run_linear(dev, ksize, stride, cins, cout, B, H, W, products, 0, variants=False, cpu32=True)
        elif epi == si.EPI_GRU_ZR:
            run_gru_zr(dev, ksize, cins[1:], cins[0], B, H, W, products, 0, cpu32=True)
        elif epi == si.EPI_GRU_Q:
            run_gru_q(dev, ksize, cins[1:], cins[0], B, H, W, products, 0, cpu32=True)
        elif epi == si.EPI_DECONV2X:
            run_deconv(dev, cins, cout // 4, B, H, W, products, 0, stats=True, cpu32=True)
        else:
            run_blend(dev, cins, B, H, W, products, 0)
    assert log and all(v == si.instance_key(p) for v in log), (name, si.instance_key(p), sorted(set(log)))
    assert s16.take_flags() == 0


# ---------------------------------------------------------------------------------------------------------------------
# the model launches nothing that the cases above did not test
# ---------------------------------------------------------------------------------------------------------------------
def test_model_launches_only_tested_instances(dev, monkeypatch, synth_weights):
    """The shipped configuration, two frames (first + temporal), 2 iterations, eager launches — 640x480, 640x480 with four sequences on
    the batch, the KITTI shape, 320x240, and hip_precision="fp16" at 640x480 — with a recorder in front of tcs_conv2d_s16: every
    launch's instance is one test_instance_vs_fp64 parametrises over.  No allow-list."""
    import bench
    from tcs_mi355 import synth
    from test_gpu_precision import _model
    tested = si.table_keys()
    log = []
    runs = [("fp32", 480, 640, 1), ("fp32", 480, 640, 4), ("fp32", 384, 1248, 1), ("fp32", 240, 320, 1), ("fp16", 480, 640, 1)]
    models = {}
    with planned(monkeypatch, log):
        for prec, H, W, nseq in runs:
            if prec not in models:
                models[prec] = _model(dev, synth_weights, hip_precision=prec)
                models[prec].use_hip_graph = False
            seqs = [synth.make_sequence(300 + j, n_frames=2, height=H, width=W, max_disp=min(192.0, W / 4)) for j in range(nseq)]
            r = bench.ClipRunner(models[prec], seqs, dev, 2)
            for _ in range(2):
                out = r.step()
            torch.cuda.synchronize()
            assert bool(torch.isfinite(out["flow"]).all()), (prec, H, W, nseq)
    seen = set(log)
    names = ("ksize", "stride", "epilogue", "taps", "products", "row_split", "rows_per_wave", "mt", "rows", "ksteps", "nstage")
    print(f"\n{len(log)} tcs_conv2d_s16 launches, {len(seen)} instances {names}:")
    for k in sorted(seen):
        print("   ", k, "" if k in tested else "   <-- NOT TESTED")
    for epi in si.EPI_NAME:
        assert any(k[2] == epi for k in seen), ("the model launched no", si.EPI_NAME[epi])
    assert {k[4] for k in seen} == {1, 3}
    missing = seen - tested
    assert not missing, sorted(missing)
