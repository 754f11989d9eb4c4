"""tcs_mi355.train_ops on the MI355X: forwards bit-equal to the value-only ops; every gradient against the float64 restatement of
test_train_ops_host.py under the project's rule e_hip <= 4 e_ref + one float32 ulp of the tensor's largest gradient, per tensor and
case, nothing excluded (e_ref: the error of the reference's own float32 gradients in tests/golden/train_ops.npz, or, for inputs the
golden file does not hold, of the same restatement in float32 on the GPU); determinism; partial gradients; what the nodes save; a
trainer-shaped step; the no-grad path and half-precision inputs."""
import numpy as np
import pytest
import torch

from test_train_ops_host import blend_restate, case_tensors, golden, restate, upsample_restate

pytestmark = pytest.mark.gpu
LEAVES = ("flow_a", "flow_b", "mask", "logits", "disp_grads")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from tcs_mi355 import native
    native.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    return golden()


def compare(tag, hip, g64, ref32):
    """The rule on one tensor, nothing excluded.  Prints the figures before it asserts."""
    hip, g64, ref32 = hip.detach().cpu().double(), g64.detach().cpu().double(), ref32.detach().cpu().double()
    assert hip.shape == g64.shape, (tag, hip.shape, g64.shape)
    assert bool(torch.isfinite(hip).all()), tag
    top = float(g64.abs().max())
    e_ref, e_hip = float((ref32 - g64).abs().max()), float((hip - g64).abs().max())
    floor = float(np.spacing(np.float32(top)))
    print(f"{tag}: max|g| {top:.3e} e_ref {e_ref:.3e} e_hip {e_hip:.3e} floor {floor:.3e}")
    assert e_hip <= 4 * e_ref + floor, (tag, e_hip, e_ref, floor)


def leaves(t):
    return {k: t[k].clone().requires_grad_(True) for k in LEAVES}


def hip_grads(t, L=None):
    """Outputs and gradients of the pair op and the blend through train_ops on the tensors of `t`."""
    from tcs_mi355 import train_ops as to
    L = L or leaves(t)
    up_a, up_b = to.upsample_flow_pair(L["flow_a"], L["flow_b"], L["mask"])
    refined = to.refine_blend(L["logits"], L["disp_grads"], t["disp"])
    dfa, dfb, dm = torch.autograd.grad([up_a, up_b], [L["flow_a"], L["flow_b"], L["mask"]], [t["g_a"], t["g_b"]])
    dl, dg = torch.autograd.grad(refined, [L["logits"], L["disp_grads"]], t["g_r"])
    return {"up_a": up_a.detach(), "up_b": up_b.detach(), "refined": refined.detach(), "dflow_a": dfa, "dflow_b": dfb, "dmask": dm,
            "dlogits": dl, "ddisp_grads": dg}


def random_case(dev, B, H, W, seed=5):
    g = torch.Generator().manual_seed(seed)
    t = {"flow_a": -(1 + 39 * torch.rand(B, 1, H, W, generator=g)), "flow_b": -(1 + 39 * torch.rand(B, 1, H, W, generator=g)),
         "mask": 2 * torch.randn(B, 144, H, W, generator=g), "g_a": torch.randn(B, 1, 4 * H, 4 * W, generator=g),
         "g_b": torch.randn(B, 1, 4 * H, 4 * W, generator=g), "logits": 2 * torch.randn(B, 9, H, W, generator=g),
         "disp_grads": 0.3 * torch.randn(B, 2, H, W, generator=g), "disp": 1 + 39 * torch.rand(B, 1, H, W, generator=g),
         "g_r": torch.randn(B, 1, H, W, generator=g)}
    return {k: v.to(dev) for k, v in t.items()}


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(5))
@pytest.mark.parametrize("grad", [False, True])
def test_forward_is_bit_equal_to_the_value_only_ops(dev, gold, i, grad):
    from tcs_mi355 import ops, train_ops as to
    t = case_tensors(gold, i, device=dev)
    L = leaves(t) if grad else t
    up_a, up_b = to.upsample_flow_pair(L["flow_a"], L["flow_b"], L["mask"])
    one_a, one_b = to.upsample_flow(L["flow_a"], L["mask"]), to.upsample_flow(L["flow_b"], L["mask"])
    refined = to.refine_blend(L["logits"], L["disp_grads"], t["disp"])
    assert up_a.requires_grad == grad and one_b.requires_grad == grad and refined.requires_grad == grad
    ref_a, ref_b = ops.convex_upsample_pair(-t["flow_a"], -t["flow_b"], t["mask"])[:2]
    assert torch.equal(up_a, ref_a) and torch.equal(up_b, ref_b)
    assert torch.equal(one_a, ops.convex_upsample(-t["flow_a"], t["mask"], clip=False)[0]) and torch.equal(one_a, up_a)
    assert torch.equal(one_b, ops.convex_upsample(-t["flow_b"], t["mask"], clip=False)[0]) and torch.equal(one_b, up_b)
    assert torch.equal(refined, ops.softmax_blend(t["logits"], ops.propagate_disparity(t["disp_grads"], t["disp"]))[0])
    # and the reference's own float32 values, to a few roundings of a 9-term sum
    for name, x in (("up_a", up_a), ("up_b", up_b), ("refined", refined)):
        ref = torch.from_numpy(gold[f"c{i}_{name}"]).to(dev)
        assert float((x - ref).abs().max()) <= 1e-5 * float(ref.abs().max()), name


@pytest.mark.parametrize("i", range(5))
def test_backward_accuracy_on_the_golden_cases(dev, gold, i):
    t = case_tensors(gold, i, device=dev)
    r64 = restate(case_tensors(gold, i, torch.float64))
    hip = hip_grads(t)
    for name in ("dflow_a", "dflow_b", "dmask", "dlogits", "ddisp_grads"):
        compare(f"c{i} {name}", hip[name], r64[name], torch.from_numpy(gold[f"c{i}_{name}"]))
    # the single op on flow_b: the same mask gradient bit for bit, the same flow gradient
    from tcs_mi355 import train_ops as to
    L = leaves(t)
    dfb, dm = torch.autograd.grad(to.upsample_flow(L["flow_b"], L["mask"]), [L["flow_b"], L["mask"]], t["g_b"])
    assert torch.equal(dm, hip["dmask"]) and torch.equal(dfb, hip["dflow_b"])


def test_backward_accuracy_on_a_larger_random_case(dev):
    t = random_case(dev, 2, 80, 180)
    r64 = restate({k: v.double() for k, v in t.items()})
    r32 = restate(t)
    hip = hip_grads(t)
    for name in ("dflow_a", "dflow_b", "dmask", "dlogits", "ddisp_grads"):
        compare(f"2x80x180 {name}", hip[name], r64[name], r32[name])


def test_determinism_and_partial_gradients(dev):
    from tcs_mi355 import train_ops as to
    t = random_case(dev, 2, 21, 37, seed=6)
    a, b = hip_grads(t), hip_grads(t)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    L = leaves(t)
    up_a, up_b = to.upsample_flow_pair(L["flow_a"], L["flow_b"], L["mask"])
    refined = to.refine_blend(L["logits"], L["disp_grads"], t["disp"])
    outs, ups = [up_a, up_b], [t["g_a"], t["g_b"]]
    for leaf, name in (("flow_a", "dflow_a"), ("flow_b", "dflow_b"), ("mask", "dmask")):
        g, = torch.autograd.grad(outs, [L[leaf]], ups, retain_graph=True)
        assert torch.equal(g, a[name]), name
    for leaf, name in (("logits", "dlogits"), ("disp_grads", "ddisp_grads")):
        g, = torch.autograd.grad(refined, [L[leaf]], t["g_r"], retain_graph=True)
        assert torch.equal(g, a[name]), name
    # a non-contiguous upstream gradient is made contiguous
    g_nc = t["g_b"].transpose(2, 3).contiguous().transpose(2, 3)
    assert not g_nc.is_contiguous()
    dm, = torch.autograd.grad(outs, [L["mask"]], [t["g_a"], g_nc], retain_graph=True)
    assert torch.equal(dm, a["dmask"])
    # double backward raises
    x = t["logits"].clone().requires_grad_(True)
    g, = torch.autograd.grad(to.refine_blend(x, t["disp_grads"], t["disp"]), x, t["g_r"], create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


def test_no_mask_gradient_buffer_when_the_mask_needs_none(dev):
    from tcs_mi355 import train_ops as to
    t = random_case(dev, 2, 40, 90, seed=7)
    mask_bytes = t["mask"].numel() * 4
    fa, fb = t["flow_a"].clone().requires_grad_(True), t["flow_b"].clone().requires_grad_(True)
    up_a, up_b = to.upsample_flow_pair(fa, fb, t["mask"])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ga, gb = torch.autograd.grad([up_a, up_b], [fa, fb], [t["g_a"], t["g_b"]])
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"backward without dmask: peak {peak} bytes over the baseline, the mask is {mask_bytes}")
    assert peak < mask_bytes // 2                       # two flow gradients + the [2,9,H,W] workspace = 20/144 of the mask
    full = hip_grads(t)
    assert torch.equal(ga, full["dflow_a"]) and torch.equal(gb, full["dflow_b"])


def test_saved_tensors(dev):
    """What the nodes keep for backward: at most the mask and both flows for the pair, the three inputs for the blend."""
    from tcs_mi355 import train_ops as to
    t = random_case(dev, 2, 20, 30, seed=8)
    L = leaves(t)
    saved = []

    def pack(x):
        saved.append(x)
        return x
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda x: x):
        to.upsample_flow_pair(L["flow_a"], L["flow_b"], L["mask"])
    nbytes = sum(x.numel() * x.element_size() for x in saved)
    assert nbytes <= 4 * (t["mask"].numel() + 2 * t["flow_a"].numel()), [tuple(x.shape) for x in saved]
    assert all(x.data_ptr() in (L["mask"].data_ptr(), L["flow_a"].data_ptr(), L["flow_b"].data_ptr()) for x in saved)
    saved.clear()
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda x: x):
        to.refine_blend(L["logits"], L["disp_grads"], t["disp"])
    nbytes = sum(x.numel() * x.element_size() for x in saved)
    assert nbytes <= 4 * (t["logits"].numel() + t["disp_grads"].numel() + t["disp"].numel()), [tuple(x.shape) for x in saved]
    assert all(x.data_ptr() in (L["logits"].data_ptr(), L["disp_grads"].data_ptr(), t["disp"].data_ptr()) for x in saved)


def test_trainer_shaped_step(dev):
    """w_head, the mask head and a two-channel gradient head on a random 128-channel feature; the tail of an iteration (blend, the
    two upsamplings on one mask) and train_losses.sequence_loss; one backward with the HIP ops and one with the restatement in
    float32, each parameter gradient held to the float64 run by the same rule."""
    from tcs_mi355 import train_losses as tl
    from tcs_mi355 import train_ops as to
    B, H, W = 2, 24, 40
    g = torch.Generator().manual_seed(9)
    feat = torch.randn(B, 128, H, W, generator=g).to(dev)
    disp = (1 + 39 * torch.rand(B, 1, H, W, generator=g)).to(dev)
    flow_q = -(disp + 0.5 * torch.randn(B, 1, H, W, generator=g).to(dev))
    flow_gt = -torch.nn.functional.interpolate(4 * disp, scale_factor=4, mode="bilinear", align_corners=True)
    flow_gt = flow_gt + torch.randn(B, 1, 4 * H, 4 * W, generator=g).to(dev)
    valid = torch.ones(B, 1, 4 * H, 4 * W, dtype=torch.bool, device=dev)

    def run(mode):
        # the float64 run is on the CPU (float64 convolutions are not a GPU library path on ROCm), the two float32 runs on the GPU
        dtype, d = (torch.float64, torch.device("cpu")) if mode == "f64" else (torch.float32, dev)
        torch.manual_seed(10)
        heads = torch.nn.ModuleDict({
            "w": torch.nn.Sequential(torch.nn.Conv2d(128, 128, 3, 1, 1), torch.nn.ReLU(), torch.nn.Conv2d(128, 9, 1)),
            "mask": torch.nn.Sequential(torch.nn.Conv2d(128, 256, 3, padding=1), torch.nn.ReLU(), torch.nn.Conv2d(256, 144, 1)),
            "grad": torch.nn.Conv2d(128, 2, 3, padding=1)}).to(d).to(dtype)
        f = feat.to(d).to(dtype)
        logits, mask, grads = heads["w"](f), 0.25 * heads["mask"](f), 0.1 * heads["grad"](f)
        if mode == "hip":
            refined = to.refine_blend(logits, grads, disp)
            up_q, up_r = to.upsample_flow_pair(flow_q, -refined, mask)
        else:
            refined = blend_restate(logits, grads, disp.to(d).to(dtype))
            up_q, up_r = upsample_restate(flow_q.to(d).to(dtype), mask.detach()), upsample_restate(-refined, mask)
        if mode == "f64":                                  # sequence_loss's terms on these predictions, in float64
            gt = flow_gt.cpu().double()
            loss = ((up_q - gt).abs() + 1.2 * (up_r - gt).abs()).mean()          # flow_mono = flow_init = gt add nothing
        else:
            loss, _ = tl.sequence_loss(flow_gt, flow_gt, [[up_q, up_r]], flow_gt, valid, [1.0])
        loss.backward()
        return float(loss), [p.grad.detach().clone() for p in heads.parameters()], [n for n, _ in heads.named_parameters()]
    l_hip, g_hip, names = run("hip")
    l_32, g_32, _ = run("f32")
    l_64, g_64, _ = run("f64")
    assert abs(l_hip - l_64) <= 1e-5 * abs(l_64), (l_hip, l_64)
    for n, a, b, c in zip(names, g_hip, g_32, g_64):
        assert float(c.abs().max()) > 0, n
        compare(f"trainer step {n}", a, c, b)


def test_no_grad_path_and_half_inputs(dev, gold):
    from tcs_mi355 import ops, train_ops as to
    t = case_tensors(gold, 1, device=dev)
    L = leaves(t)
    with torch.no_grad():
        up_a, up_b = to.upsample_flow_pair(L["flow_a"], L["flow_b"], L["mask"])
        one = to.upsample_flow(L["flow_b"], L["mask"])
        refined = to.refine_blend(L["logits"], L["disp_grads"], t["disp"])
    assert not (up_a.requires_grad or up_b.requires_grad or one.requires_grad or refined.requires_grad)
    assert up_a.grad_fn is None and refined.grad_fn is None
    ref_a, ref_b = ops.convex_upsample_pair(-t["flow_a"], -t["flow_b"], t["mask"])[:2]
    assert torch.equal(up_a, ref_a) and torch.equal(up_b, ref_b) and torch.equal(one, ref_b)
    assert torch.equal(refined, ops.softmax_blend(t["logits"], ops.propagate_disparity(t["disp_grads"], t["disp"]))[0])
    for half in (torch.float16, torch.bfloat16):
        m16 = t["mask"].to(half).requires_grad_(True)
        up = to.upsample_flow(t["flow_b"], m16)
        assert up.dtype == torch.float32 and torch.equal(up, to.upsample_flow(t["flow_b"], m16.detach().float()))
        gm, = torch.autograd.grad(up, m16, t["g_b"])
        assert gm.dtype == half and gm.shape == m16.shape
        m32 = m16.detach().float().requires_grad_(True)
        g32, = torch.autograd.grad(to.upsample_flow(t["flow_b"], m32), m32, t["g_b"])
        assert torch.equal(gm, g32.to(half))
        l16 = t["logits"].to(half).requires_grad_(True)
        r = to.refine_blend(l16, t["disp_grads"], t["disp"])
        assert r.dtype == torch.float32 and torch.equal(r, to.refine_blend(l16.detach().float(), t["disp_grads"], t["disp"]))


def test_patched_reference_shaped_modules(dev):
    """patch_reference on stand-ins with the reference's attribute names: the patched forward returns refine_blend's value on the
    module's own w_head and the 0.25-scaled mask, and gradients reach w_head and disp_grads."""
    from types import SimpleNamespace

    from tcs_mi355 import ops, train_ops as to

    class TCStereo(torch.nn.Module):
        def upsample_flow(self, flow, mask, scale=True):
            raise AssertionError("the original must not run for scale=True")

    class DispRefine(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.context_compress = torch.nn.Conv2d(192, 96, 3, 1, 1)
            self.disp_f_stem = torch.nn.Conv2d(27, 96, 1)
            self.conv_fuse = torch.nn.Conv2d(192, 128, 3, 1, 1)
            self.w_head = torch.nn.Conv2d(128, 9, 1)
            self.mask = torch.nn.Conv2d(128, 144, 1)

        def forward(self, *a, **k):
            raise AssertionError("the original must not run")
    undo = to.patch_reference(SimpleNamespace(TCStereo=TCStereo), SimpleNamespace(DispRefine=DispRefine))
    try:
        torch.manual_seed(11)
        B, H, W = 1, 12, 20
        m = DispRefine().to(dev)
        grads = (0.3 * torch.randn(B, 2, H, W, device=dev)).requires_grad_(True)
        disp = 1 + 39 * torch.rand(B, 1, H, W, device=dev)
        cd, cg = torch.randn(B, 128, H, W, device=dev), torch.randn(B, 64, H, W, device=dev)
        refined, mask = m(grads, disp, cd, cg)
        with torch.no_grad():
            stem = ops.propagate_disparity(grads.detach(), disp)
            fused = m.conv_fuse(torch.cat((m.disp_f_stem(stem), m.context_compress(torch.cat((cd, cg), 1))), 1))
            assert torch.equal(refined, ops.softmax_blend(m.w_head(fused).contiguous(), stem)[0])
            assert torch.equal(mask, 0.25 * m.mask(fused))
        assert m(grads, disp, cd, cg, test_mode=True)[1] is None
        tc = TCStereo()
        tc.args = SimpleNamespace(n_downsample=2)
        flow = -disp
        up = tc.upsample_flow(flow, mask)
        assert torch.equal(up, to.upsample_flow(flow, mask))
        up.sum().backward(retain_graph=True)
        assert grads.grad is None and m.mask.weight.grad is not None and m.w_head.weight.grad is None
        refined.sum().backward()
        assert grads.grad is not None and m.w_head.weight.grad is not None and float(grads.grad.abs().max()) > 0
    finally:
        undo()
