"""Gradients of CorrBlock1D on the MI355X (k_corr_lookup_bwd, k_corr_gemm_bwd, k_corr_norm_bwd through tcs_mi355.corr): every
differentiable output against the oracle's fp64 autograd, with the bar tied to the reference formulation's own fp32 error on the
same device (test_corr_grad_host.grad_error_ok); the golden; determinism and partial backwards; forward bits unchanged by grad
mode; the training shape; and a small trainer step through a conv feature net."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from test_corr_grad_host import (_leaves, _score, fmap_groups, golden, golden_case, grad_error_ok, oracle_grads,
                                 torch_reference_block, torch_reference_grads)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from tcs_mi355 import native
    native.lib()
    return torch.device("cuda:0")


def hip_grads(case, radius, dev, lookups=None, cost=True, main=True, coords_grad=True):
    from tcs_mi355.corr import CorrBlock1D
    lookups = case["coords"].shape[0] if lookups is None else lookups
    f1, f2, coords = _leaves(case, torch.float32, dev, lookups)
    if not coords_grad:
        coords = [c.detach() for c in coords]
    blk = CorrBlock1D(f1, f2, radius=radius, want_argmax=main, want_cost_volume=cost)
    outs = [blk(c) for c in coords]
    loss = _score(case, outs, blk.get_cost_volume() if cost else None, blk.argmax_disp()[1] if main else None, dev, torch.float32)
    inputs = [f1, f2] + (coords if coords_grad else [])
    g = torch.autograd.grad(loss, inputs)
    return g[0], g[1], list(g[2:])


def check_all(case, radius, dev, oracle, lookups=None, cost=True, main=True, coords_grad=True):
    h1, h2, hc = hip_grads(case, radius, dev, lookups, cost, main, coords_grad)
    o1, o2, oc = oracle_grads(oracle, case, radius, lookups, cost, main)
    t1, t2, tc = torch_reference_grads(case, radius, dev, lookups, cost, main)
    for name, h, t, o, f in (("fmap1", h1, t1, o1, case["fmap1"]), ("fmap2", h2, t2, o2, case["fmap2"])):
        ok, msg = grad_error_ok(h, t, o, fmap_groups(f))
        assert ok, (name, msg)
        assert float(o.abs().max()) > 0, name
    for k, (h, t, o) in enumerate(zip(hc, tc, oc)):
        ok, msg = grad_error_ok(h, t, o)
        assert ok, ("coords", k, msg)


@pytest.mark.parametrize("B,W,radius", [(1, 40, 4), (2, 100, 4), (4, 160, 4), (2, 40, 2), (1, 100, 7)])
def test_lookup_grads_vs_oracle(dev, oracle, B, W, radius):
    """Three lookups (fractional, out-of-range, integer with +-1000 and +-3e9) -> fmap1, fmap2, coords."""
    from tcs_mi355 import synth
    case = synth.make_corr_grad_case(100 + B * W + radius, B, 256, 3, W, radius)
    check_all(case, radius, dev, oracle, cost=False, main=False)


def test_five_detached_lookups(dev, oracle):
    """The reference's loop: coords1 is detached before every lookup (tc_stereo.py:175-177); one backward sums all five."""
    from tcs_mi355 import synth
    case = synth.make_corr_grad_case(7, 2, 256, 4, 72, 4, lookups=5)
    check_all(case, 4, dev, oracle, cost=False, main=False, coords_grad=False)


@pytest.mark.parametrize("cost,main", [(True, False), (False, True), (True, True)])
def test_cost_volume_and_main_cost(dev, oracle, cost, main):
    from tcs_mi355 import synth
    case = synth.make_corr_grad_case(21, 2, 256, 3, 52, 4, lookups=1)
    check_all(case, 4, dev, oracle, lookups=1 if cost else 0, cost=cost, main=main)
    from tcs_mi355.corr import CorrBlock1D
    f = torch.from_numpy(case["fmap1"]).to(dev).requires_grad_(True)
    m = CorrBlock1D(f, torch.from_numpy(case["fmap2"]).to(dev)).argmax_disp()[2]
    assert float(m.mean()) > 0.5                     # the margin mask is mostly on: main_cost carries gradient


def test_golden(dev):
    g = golden()
    case, r = golden_case(g)
    h1, h2, hc = hip_grads(case, r, dev)
    for h, ref, f in ((h1, g["grad_fmap1"], case["fmap1"]), (h2, g["grad_fmap2"], case["fmap2"])):
        for m in fmap_groups(f):
            m = m.expand(*ref.shape).numpy()
            d = np.abs(h.cpu().numpy()[m] - ref[m]).max()
            assert d <= 2e-5 * np.abs(ref[m]).max(), d
    kink = (np.round(case["coords"]) == case["coords"]) & (np.abs(case["coords"]) < 1000)
    hc = np.stack([c.cpu().numpy() for c in hc])
    d = np.abs(hc - g["grad_coords"])[~kink].max()
    assert d <= 2e-5 * np.abs(g["grad_coords"]).max(), d


def _corr_and_static_loss(f1, f2, gv, gp):
    from tcs_mi355.corr import CorrBlock1D
    v = CorrBlock1D.corr(f1, f2)
    blk = CorrBlock1D(f1, f2)
    loss = (v * gv).sum()
    for lv, g in zip(blk.corr_pyramid, gp):
        loss = loss + (lv * g).sum()
    return loss


def test_corr_and_pyramid_paths(dev, oracle):
    from tcs_mi355 import synth
    case = synth.make_corr_grad_case(5, 2, 256, 3, 44, 4, lookups=1)
    B, C, H, W = case["fmap1"].shape
    gen = torch.Generator().manual_seed(3)
    gv = torch.randn(B, H, W, 1, W, generator=gen, dtype=torch.float64)
    gp = [torch.randn(B * H * W, 1, 1, W >> i, generator=gen, dtype=torch.float64) for i in range(4)]

    def run(f1, f2, vol_fn, pyr_fn):
        v = vol_fn(f1, f2)
        loss = (v.reshape(B, H, W, 1, W) * gv.to(v)).sum()
        for lv, g in zip(pyr_fn(v), gp):
            loss = loss + (lv.reshape(B * H * W, 1, 1, -1) * g.to(lv)).sum()
        return torch.autograd.grad(loss, [f1, f2])

    f1, f2, _ = _leaves(case, torch.float32, dev, 0)
    h = torch.autograd.grad(_corr_and_static_loss(f1, f2, gv.to(dev, torch.float32), [g.to(dev, torch.float32) for g in gp]),
                            [f1, f2])
    o = run(*_leaves(case, torch.float64, "cpu", 0)[:2], oracle.corr_volume, oracle.corr_pyramid)

    def ref_vol(a, b):
        import torch.nn.functional as F
        return torch.einsum('aijk,aijh->ajkh', F.normalize(a, dim=1), F.normalize(b, dim=1))

    def ref_pyr(v):
        import torch.nn.functional as F
        p = [v.reshape(B * H * W, 1, 1, W)]
        for _ in range(3):
            p.append(F.avg_pool2d(p[-1], [1, 2], stride=[1, 2]))
        return p

    t = run(*_leaves(case, torch.float32, dev, 0)[:2], ref_vol, ref_pyr)
    for i, f in enumerate((case["fmap1"], case["fmap2"])):
        ok, msg = grad_error_ok(h[i], t[i], o[i], fmap_groups(f))
        assert ok, (i, msg)


def _full_backward(case, dev, retain=False, twice=False, coords_first=False):
    from tcs_mi355.corr import CorrBlock1D
    f1, f2, coords = _leaves(case, torch.float32, dev, case["coords"].shape[0])
    blk = CorrBlock1D(f1, f2, want_cost_volume=True)
    outs = [blk(c) for c in coords]
    loss = _score(case, outs, blk.get_cost_volume(), blk.argmax_disp()[1], dev, torch.float32)
    res = []
    if coords_first:
        gc = torch.autograd.grad(loss, coords, retain_graph=True)
        res.append([g.clone() for g in gc])
    loss.backward(retain_graph=retain)
    res.append([t.grad.clone() for t in [f1, f2, *coords]])
    if twice:
        for t in [f1, f2, *coords]:
            t.grad = None
        loss.backward()
        res.append([t.grad.clone() for t in [f1, f2, *coords]])
    return res


def test_determinism_retain_graph_and_partial_backward(dev, oracle):
    from tcs_mi355 import synth
    case = synth.make_corr_grad_case(9, 2, 256, 3, 60, 4)
    a = _full_backward(case, dev)[0]
    b = _full_backward(case, dev)[0]
    for x, y in zip(a, b):
        assert torch.equal(x, y)                                    # two backwards: bit-equal
    r = _full_backward(case, dev, retain=True, twice=True)
    for x, y in zip(r[0], r[1]):
        assert torch.equal(x, y)                                    # retain_graph: the same gradients twice
    p = _full_backward(case, dev, coords_first=True)
    for x, y in zip(p[0], a[2:]):
        assert torch.equal(x, y)                                    # autograd.grad w.r.t. coords only
    for x, y in zip(p[1], a):
        assert torch.equal(x, y)                                    # ... leaves nothing behind for the full backward
    o = oracle_grads(oracle, case, 4)
    for x, y, f in zip(a[:2], o[:2], (case["fmap1"], case["fmap2"])):
        g = fmap_groups(f)[0].expand_as(y)
        assert float((x.cpu().double() - y)[g].abs().max()) <= 1e-4 * float(y[g].abs().max())


def test_double_backward_raises(dev):
    from tcs_mi355 import synth
    from tcs_mi355.corr import CorrBlock1D
    case = synth.make_corr_grad_case(2, 1, 256, 2, 40, 4, lookups=1)
    f1, f2, coords = _leaves(case, torch.float32, dev, 1)
    out = CorrBlock1D(f1, f2)(coords[0])
    g, = torch.autograd.grad(out.sum(), f1, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


def test_forward_bits_unchanged_by_grad_mode(dev):
    from tcs_mi355 import synth
    from tcs_mi355.corr import CorrBlock1D
    case = synth.make_corr_grad_case(4, 2, 256, 3, 100, 4)
    f1, f2, coords = _leaves(case, torch.float32, dev, 3)
    blk_g = CorrBlock1D(f1, f2, want_cost_volume=True)
    with torch.no_grad():
        blk_n = CorrBlock1D(f1, f2, want_cost_volume=True)
        ref = [blk_n(c) for c in coords] + [blk_n.get_cost_volume()] + list(blk_n.argmax_disp())
        ref += list(blk_n.corr_pyramid) + [CorrBlock1D.corr(f1, f2)]
    got = [blk_g(c) for c in coords] + [blk_g.get_cost_volume()] + list(blk_g.argmax_disp())
    got += list(blk_g.corr_pyramid) + [CorrBlock1D.corr(f1, f2)]
    assert got[0].grad_fn is not None and got[3].grad_fn is not None and got[5].grad_fn is not None
    for x, y in zip(got, ref):
        assert y.grad_fn is None
        assert torch.equal(x.detach(), y)


def test_fp16_inputs_cast_differentiably(dev):
    from tcs_mi355 import synth
    from tcs_mi355.corr import CorrBlock1D
    case = synth.make_corr_grad_case(6, 1, 256, 2, 48, 4, lookups=1)
    f1 = torch.from_numpy(case["fmap1"]).to(dev).half().requires_grad_(True)
    f2 = torch.from_numpy(case["fmap2"]).to(dev).half().requires_grad_(True)
    out = CorrBlock1D(f1, f2)(torch.from_numpy(case["coords"][0]).to(dev).half())
    assert out.dtype == torch.float32
    out.sum().backward()
    assert f1.grad.dtype == torch.float16 and torch.isfinite(f1.grad[:, :, 1:]).all() and float(f2.grad.abs().max()) > 0


def test_training_shape(dev, oracle):
    """B=4, C=256, 120x160 (a 480x640 crop at 1/4), five lookups at detached coords plus the cost volume."""
    from tcs_mi355 import synth
    case = synth.make_corr_grad_case(12, 4, 256, 120, 160, 4, lookups=5)
    check_all(case, 4, dev, oracle, lookups=5, cost=True, main=False, coords_grad=False)


class _Feat(nn.Module):
    def __init__(self):
        super().__init__()
        self.c1 = nn.Conv2d(3, 32, 3, padding=1)
        self.c2 = nn.Conv2d(32, 256, 3, padding=1)

    def forward(self, x):
        return self.c2(torch.relu(self.c1(x)))


def test_tiny_trainer_step(dev, oracle):
    """A conv feature net feeds the correlation; two lookups and the cost volume go into an L1 loss.  Parameter gradients of the
    HIP step against the same net with the oracle's correlation in fp64 (bar: the reference formulation in fp32 on the GPU)."""
    from tcs_mi355.corr import CorrBlock1D
    torch.manual_seed(0)
    net = _Feat()
    gen = torch.Generator().manual_seed(1)
    B, H, W, r = 2, 6, 56, 4
    im1 = torch.randn(B, 3, H, W, generator=gen)
    im2 = torch.roll(im1, -5, dims=3) + 0.2 * torch.randn(B, 3, H, W, generator=gen)
    coords = [torch.arange(W).view(1, 1, 1, W).expand(B, 1, H, W) - 5 + 0.7 * torch.randn(B, 1, H, W, generator=gen)
              for _ in range(2)]
    tgt_l = [torch.randn(B, 4 * (2 * r + 1), H, W, generator=gen) for _ in range(2)]
    tgt_c = torch.randn(B, W, H, W, generator=gen)

    def step(device, dtype, kind):
        m = _Feat().to(device=device, dtype=dtype)
        m.load_state_dict(net.state_dict())
        f1, f2 = m(im1.to(device, dtype)), m(im2.to(device, dtype))
        cs = [c.to(device, dtype) for c in coords]
        if kind == "hip":
            blk = CorrBlock1D(f1, f2, want_argmax=False, want_cost_volume=True)
            outs, cv = [blk(c) for c in cs], blk.get_cost_volume()
        elif kind == "torch":
            lookup, cv, _ = torch_reference_block(f1, f2, r)
            outs = [lookup(c) for c in cs]
        else:
            vol = oracle.corr_volume(f1, f2)
            pyr = oracle.corr_pyramid(vol)
            outs, cv = [oracle.corr_lookup(pyr, c, r) for c in cs], oracle.masked_cost_volume(vol)
        loss = sum((o - t.to(device, dtype)).abs().mean() for o, t in zip(outs, tgt_l)) + (cv - tgt_c.to(device, dtype)).abs().mean()
        return torch.autograd.grad(loss, list(m.parameters()))

    h = step(dev, torch.float32, "hip")
    t = step(dev, torch.float32, "torch")
    o = step("cpu", torch.float64, "oracle")
    for i, (a, b, c) in enumerate(zip(h, t, o)):
        ok, msg = grad_error_ok(a, b, c)
        assert ok, (i, msg)
        assert float(c.abs().max()) > 0
