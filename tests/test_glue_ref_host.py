"""CPU: the float64 restatements of tests/glue_ref.py are what the reference computes — so that test_gpu_glue_fp64.py, which compares the HIP
kernels with them, certifies the kernels and not itself.  Three anchors: the reference-generated arrays of tests/golden/ops_small.npz
(tolerances of test_oracle_golden.py for the same arrays), the oracle's functions on two random ragged shapes, and — for the operators
the oracle only has inline — PyTorch's own operators in float64.  Also the conditions on the inputs that the GPU tests rely on."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import glue_ref as gr
from conftest import T, maxdiff

RAGGED = [(2, 7, 13), (1, 19, 6)]


def test_restatements_against_reference_goldens(ops_golden):
    g = ops_golden
    d = T(g["geo_disp"])
    # the goldens are float32: a float64 difference of two float32 values is exact, and rounded to float32 it is the float32 difference
    assert maxdiff(gr.grad_xy(d).float(), g["geo_grad_xy"]) == 0
    ref = g["geo_grad_cands"]
    n, _, _, h, w = ref.shape
    ref = ref.reshape(n, 32, h, w)
    got = gr.grad_candidates(d).numpy()
    fin = np.isfinite(ref)
    assert (np.isfinite(got) == fin).all()
    assert np.abs(got[fin] - ref[fin]).max() <= 1e-5 * max(1.0, np.abs(ref[fin]).max())
    p27 = gr.propagate(T(g["prop_grad"]), T(g["prop_disp"]))
    assert maxdiff(p27[:, :9], g["prop_cand"]) <= 1e-6
    assert maxdiff(p27[:, 9:].float(), g["prop_matrix"]) == 0
    flow, mask = T(g["ups_flow"]), T(g["ups_mask"])
    # ups_out (|values| up to ~60) carries the reference's float32 rounding, ~1e-5: the oracle's 2e-6 holds for the float32 evaluation,
    # the float64 one is within the 1e-5 the GPU golden test allows for this array
    with gr.evaluated_in(torch.float32):
        assert maxdiff(gr.upsample_flow(flow, mask), g["ups_out"]) <= 2e-6
        up, fq = gr.convex_upsample(-flow, mask, clip=False)            # the disparity form of the same call
        assert maxdiff(up, g["ups_out"]) <= 2e-6 and maxdiff(fq, flow) == 0
        upc, fqc = gr.convex_upsample(-flow, mask, clip=True)
        assert maxdiff(upc, np.minimum(g["ups_out"], 0)) <= 2e-6 and maxdiff(fqc, flow.clamp(max=0)) == 0
    assert gr.upsample_flow(flow, mask).dtype == torch.float64 and maxdiff(gr.upsample_flow(flow, mask), g["ups_out"]) <= 1e-5


@pytest.mark.parametrize("shape", RAGGED)
def test_restatements_against_oracle(oracle, shape):
    B, H, W = shape
    d, g = gr.disparity(B, H, W).double(), gr.gradient(B, H, W).double()
    assert maxdiff(gr.grad_xy(d, 5.0), 5.0 * oracle.disp_gradient_xy(d)) == 0
    assert maxdiff(gr.grad_candidates(d), oracle.grad_candidates(d).reshape(B, 32, H, W)) == 0
    cand, mat = oracle.propagate_disparity(g, d)
    assert maxdiff(gr.propagate(g, d), torch.cat([cand, mat], 1)) == 0
    mask = gr.logits(B, 144, H, W).double()
    assert maxdiff(gr.upsample_flow(-d, mask), oracle.convex_upsample(-d, mask, 4)) == 0
    assert maxdiff(gr.convex_upsample(d, mask, True)[0], oracle.convex_upsample(-d, mask, 4).clamp(max=0)) == 0
    # the loop's bookkeeping as tc_stereo_forward spells it (coords0 = the column index)
    c1, dl = gr.coords_and_delta(B, H, W)
    c0 = torch.arange(W, dtype=torch.float64).view(1, 1, 1, W).expand(B, 1, H, W)
    new_c1, dq = gr.flow_step(c1, dl)
    assert maxdiff(new_c1, c1.double() + dl.double()) == 0 and maxdiff(dq, c0 - (c1.double() + dl.double())) == 0
    dq2, g2, c2 = gr.flow_step_grads(c1, dl, 5.0)
    assert maxdiff(dq2, dq) == 0 and maxdiff(g2, 5.0 * oracle.disp_gradient_xy(dq)) == 0
    assert maxdiff(c2, oracle.grad_candidates(dq).reshape(B, 32, H, W)) == 0
    # the blend: disp_refine's lines (softmax over the 9 logits, weighted candidates) + coords1 = coords0 - refined
    lg = gr.logits(B, 9, H, W).double()
    wgt = torch.softmax(lg - lg.max(dim=1, keepdim=True)[0], dim=1)
    want = (wgt * cand).sum(1, keepdim=True)
    r, dlt, co, fx = gr.softmax_blend(lg, gr.propagate(g, d), d)
    assert maxdiff(r, want) <= 1e-12 and maxdiff(dlt, want - d) <= 1e-12
    assert maxdiff(co, c0 - want) <= 1e-12 and maxdiff(fx, -want) <= 1e-12
    # pool / resize: the oracle's update-block glue
    x = gr.hidden(B, 5, H, W).double()
    assert maxdiff(gr.avgpool3s2(x), oracle._pool2x(x)) <= 1e-15
    for Ho, Wo in (gr.resize_target(H, W), (H + 3, 2 * W), (1, 1), (H, W)):
        like = torch.empty(1, 1, Ho, Wo)
        assert maxdiff(gr.resize_bilinear(x, Ho, Wo), oracle._interp(x, like)) <= 1e-14, (Ho, Wo)
        assert maxdiff(gr.resize_bilinear(x, Ho, Wo, scale=-4.0), -4.0 * oracle._interp(x, like)) <= 1e-13


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 2, 3), (1, 3, 2), (1, 1, 9), (1, 9, 1)])
def test_pool_resize_degenerate_sizes(shape):
    B, H, W = shape
    x = gr.hidden(B, 3, H, W).double()
    assert maxdiff(gr.avgpool3s2(x), F.avg_pool2d(x, 3, stride=2, padding=1)) <= 1e-15
    Ho, Wo = gr.resize_target(H, W)
    assert maxdiff(gr.resize_bilinear(x, Ho, Wo), F.interpolate(x, (Ho, Wo), mode="bilinear", align_corners=True)) <= 1e-14


@pytest.mark.parametrize("nout", (1, 2))
def test_taps_sum_is_the_folded_convolution(nout):
    """Tap partials built in float64 the way their producer defines them (per 32-channel tile, per weight tap, at the source pixel):
    their sum is conv2d(y, w, b, padding=1)."""
    gen = torch.Generator().manual_seed(5 + nout)
    B, ntile, H, W = 2, 3, 6, 11
    y = torch.randn(B, 32 * ntile, H, W, generator=gen, dtype=torch.float64)
    w = torch.randn(nout, 32 * ntile, 3, 3, generator=gen, dtype=torch.float64)
    b = torch.randn(nout, generator=gen, dtype=torch.float64)
    add = torch.randn(B, nout, H, W, generator=gen, dtype=torch.float64)
    yt = y.view(B, ntile, 32, H, W)
    wt = w.view(nout, ntile, 32, 9)
    planes = torch.einsum("bkchw,okct->bkothw", yt, wt).reshape(B, ntile, nout * 9, H, W)
    ref = F.conv2d(y, w, b, padding=1)
    assert maxdiff(gr.taps_sum(planes, nout, b), ref) <= 1e-12
    assert maxdiff(gr.taps_sum(planes, nout, b, add, 0.2), (ref + add) * 0.2) <= 1e-12
    assert maxdiff(gr.taps_sum(planes, nout), F.conv2d(y, w, None, padding=1)) <= 1e-12


@pytest.mark.parametrize("act", gr.ACTS)
def test_instance_norm_restatement(act):
    x = gr.ramped_planes(2, 5, 9, 14).double()
    add = gr.hidden(2, 5, 9, 14).double()
    n = F.instance_norm(x, eps=1e-5)
    want = {"none": n, "relu": torch.relu(n), "leaky": F.leaky_relu(n, 0.01), "relu_add_relu": torch.relu(n)}[act] + add
    if act == "relu_add_relu":
        want = torch.relu(want)
    assert maxdiff(gr.instance_norm(x, act, add), want) <= 1e-13
    assert maxdiff(gr.instance_norm(x, "none", None, eps=1e-3), F.instance_norm(x, eps=1e-3)) <= 1e-13


def test_input_conditions():
    """What the GPU cases assume of their inputs, checked where it is cheap."""
    for B, H, W in gr.FIELDS + gr.TAP_FIELDS:
        d = gr.disparity(B, H, W)
        assert float(d.min()) >= 0 and float(d.max()) <= 40
        assert bool(torch.isfinite(gr.grad_candidates(d)).all())            # finite everywhere: no pixel is left out of a comparison
        lg = gr.logits(B, 9, H, W)
        assert float((lg[B - 1, :, H - 1, W // 2] - 0.75).abs().max()) == 0
    # slice lengths of the S16 InstanceNorm planes: a single partly filled slice, one exactly full, short last slices, two full ones
    assert [gr.in_slices(h * w) for h, w in gr.IN_PLANES] == [[63], [2560], [1281, 1280], [1312, 1311], [1728, 1728, 1727], [2560, 2560]]
    for H, W in gr.IN_PLANES:
        if len(gr.in_slices(H * W)) > 1:
            assert gr.between_slice_share(gr.ramped_planes(2, 24, H, W)) > 0.5, (H, W)
            assert gr.between_slice_share(gr.ramped_planes(2, 24, H, W, ramp=0.0)) < 0.05       # what i.i.d. noise gives the merge
    assert gr.between_slice_share(gr.ramped_planes(2, 24, 71, 73, ramp=4.0, sigma=0.5, offset=8.0)) > 0.5
