"""Float64 restatements of the refinement loop's stencil and glue operators, and the inputs the glue tests run them on — ONE place,
read by test_glue_ref_host.py (which pins every function below to the reference-generated goldens, to the oracle and to PyTorch's own
operators, on the CPU) and by test_gpu_glue_fp64.py (which compares the HIP kernels with them).

Written from the reference's formulas (core/utils/geo_utils.py:73-132, core/update.py:259-300, core/tc_stereo.py:75-88, 188-213,
core/update.py:114-124, core/utils/basic_layers.py:28-35), not from the kernels.  Where oracle/tcs_oracle.py has the operator it is
called (it is dtype-generic); everything else is spelled out with pads, slices and gathers, so that the host test can hold it against
the library operator (F.avg_pool2d, F.interpolate, F.instance_norm, F.conv2d, torch.softmax) as a second, independent statement.
Every function takes tensors of any float dtype on any device and returns float64 CPU tensors."""
import contextlib
import os
import sys

import torch
import torch.nn.functional as F

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "oracle"))
import tcs_oracle as oracle  # noqa: E402


_DTYPE = [torch.float64]


def f64(x):
    return x.detach().cpu().to(_DTYPE[0])


@contextlib.contextmanager
def evaluated_in(dtype):
    """Evaluate the restatements in `dtype` instead of float64: the goldens were computed by the reference in float32 and carry its
    rounding, so the host test holds the float32 evaluation against them at the oracle's float32 tolerances."""
    _DTYPE.insert(0, dtype)
    try:
        yield
    finally:
        _DTYPE.pop(0)


def _xs(like):
    return torch.arange(like.shape[-1], dtype=_DTYPE[0]).view(1, 1, 1, -1)


# ---------------------------------------------------------------------------------------------------------------------
# operators
# ---------------------------------------------------------------------------------------------------------------------
def flow_step(coords1, delta):
    """tc_stereo.py:188-189 -> (coords1 + delta, disp_q = coords0 - coords1), coords0 = the pixel's column."""
    c = f64(coords1) + f64(delta)
    return c, _xs(c) - c


def grad_xy(disp, scale=1.0):
    """geo_utils.py:115-132 (times `scale`: update.py:207 feeds the predictor 5 * gradient)."""
    return scale * oracle.disp_gradient_xy(f64(disp))


def grad_candidates(disp):
    """geo_utils.py:73-101, level 2, as the 32 channels [x components of the 16 candidates | y components]."""
    g = oracle.grad_candidates(f64(disp))
    n, _, _, h, w = g.shape
    return g.reshape(n, 32, h, w)


def flow_step_grads(coords1, delta, scale=1.0):
    """The three stencils of an iteration on disp_q = x - (coords1 + delta) -> (disp_q, scale * gradient, candidates)."""
    _, dq = flow_step(coords1, delta)
    return dq, grad_xy(dq, scale), grad_candidates(dq)


def propagate(grad, disp):
    """update.py:259-289 -> the 27 channels cat(9 candidates, |g_c - g_n| x (9), |g_c - g_n| y (9))."""
    cand, mat = oracle.propagate_disparity(f64(grad), f64(disp))
    return torch.cat([cand, mat], 1)


def softmax_blend(logits, cand, disp_q):
    """update.py:298-300 + tc_stereo.py:198-202, 178 -> (refined, delta = refined - disp_q, coords1 = coords0 - refined,
    flow_x = coords1 - coords0).  `cand` may carry more than 9 channels (the 27-channel stem input): the first 9 are used."""
    l, c = f64(logits), f64(cand)[:, :9]
    e = torch.exp(l - l.max(dim=1, keepdim=True)[0])
    refined = ((e / e.sum(dim=1, keepdim=True)) * c).sum(1, keepdim=True)
    coords1 = _xs(refined) - refined
    return refined, refined - f64(disp_q), coords1, coords1 - _xs(refined)


def upsample_flow(flow, mask):
    """tc_stereo.py:75-88 at factor 4: the flow form."""
    return oracle.convex_upsample(f64(flow), f64(mask), 4)


def convex_upsample(disp, mask, clip):
    """The disparity form: upsample_flow(-disp) and flow_q = -disp, both clamped to <= 0 when `clip` (tc_stereo.py:220-224)."""
    up, fq = upsample_flow(-f64(disp), mask), -f64(disp)
    return (up.clamp(max=0), fq.clamp(max=0)) if clip else (up, fq)


def avgpool3s2(x):
    """update.py:114-115: 3x3 window, stride 2, zero padding 1, divisor always 9."""
    x = f64(x)
    H, W = x.shape[-2:]
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    p = F.pad(x, (1, 1, 1, 1))
    acc = 0
    for v in range(3):
        for u in range(3):
            acc = acc + p[..., v:v + 2 * Ho - 1:2, u:u + 2 * Wo - 1:2]
    return acc / 9


def resize_bilinear(x, Ho, Wo, scale=None):
    """update.py:122-124: bilinear, align_corners=True (output i samples input i * (n - 1) / (no - 1)); times `scale` when given."""
    x = f64(x)
    H, W = x.shape[-2:]

    def axis(n, no):
        pos = torch.arange(no, dtype=torch.float64) * ((n - 1) / (no - 1) if no > 1 else 0.0)
        i0 = pos.floor().clamp(0, n - 1).long()
        return i0, (i0 + 1).clamp(max=n - 1), pos - i0

    y0, y1, ly = axis(H, Ho)
    x0, x1, lx = axis(W, Wo)
    ly, lx = ly.view(-1, 1), lx.view(1, -1)
    top = x[..., y0, :][..., x0] * (1 - lx) + x[..., y0, :][..., x1] * lx
    bot = x[..., y1, :][..., x0] * (1 - lx) + x[..., y1, :][..., x1] * lx
    out = top * (1 - ly) + bot * ly
    return out if scale is None else out * scale


def taps_sum(planes, nout, bias=None, addend=None, scale=1.0):
    """A 3x3 convolution to `nout` channels from its tap partials (update.py:13-17, 196, 213 folded into the producer):
    planes [B, ntile, nout*9, H, W], plane o*9 + t holds the products with weight tap t = 3*ky + kx at the SOURCE pixel, so
    out[o][y][x] = (addend + bias[o] + sum_tiles sum_t planes[o*9 + t][y + ky - 1][x + kx - 1]) * scale, zero outside the image."""
    P = f64(planes).sum(1)                                      # [B, nout*9, H, W]
    B, _, H, W = P.shape
    pp = F.pad(P, (1, 1, 1, 1))
    out = torch.zeros(B, nout, H, W, dtype=P.dtype)
    for o in range(nout):
        for t in range(9):
            out[:, o] += pp[:, o * 9 + t, t // 3:t // 3 + H, t % 3:t % 3 + W]
    if bias is not None:
        out = out + f64(bias).view(1, nout, 1, 1)
    if addend is not None:
        out = out + f64(addend)
    return out * scale


ACTS = ("none", "relu", "leaky", "relu_add_relu")


def instance_norm(x, act="none", addend=None, eps=1e-5):
    """InstanceNorm2d(affine=False): biased variance over the plane (basic_layers.py:28-35), then the activation, then the addend;
    relu_add_relu = relu(relu(norm) + addend), the extractor's residual form (extractor.py:44-58)."""
    x = f64(x)
    mean = x.mean(dim=(2, 3), keepdim=True)
    var = ((x - mean) ** 2).mean(dim=(2, 3), keepdim=True)
    y = (x - mean) / torch.sqrt(var + eps)
    if act in ("relu", "relu_add_relu"):
        y = y.clamp(min=0)
    elif act == "leaky":
        y = torch.where(y > 0, y, 0.01 * y)
    elif act != "none":
        raise ValueError(act)
    if addend is not None:
        y = y + f64(addend)
    return y.clamp(min=0) if act == "relu_add_relu" else y


# ---------------------------------------------------------------------------------------------------------------------
# inputs (deterministic; the host test checks the conditions the GPU tests rely on)
# ---------------------------------------------------------------------------------------------------------------------
# every per-pixel fp32 stencil: all-border sizes, exactly one 256-thread block, a row / a column crossing a block boundary, a block
# boundary in the middle of a row with batch 2, 11 blocks with a partial last one
FIELDS = [(1, 1, 1), (1, 2, 3), (1, 3, 2), (2, 16, 16), (1, 1, 257), (1, 257, 1), (2, 17, 31), (3, 41, 67)]
UPSAMPLE_FIELDS = [f for f in FIELDS if f != (1, 257, 1)]       # blocks count 16*H*W there: (1,1,257) already is a 16-block strip
S16_FIELDS = [f for f in FIELDS if f[1] >= 2 and f[2] >= 2]
TAP_FIELDS = [(1, 3, 5), (1, 8, 16), (2, 9, 17), (1, 7, 33), (2, 24, 48)]      # 16x8 LDS tiles: below one, exactly one, ragged, several


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def disparity(B, H, W, seed=0):
    """Random in [0, 40] with one discontinuity column (a 20-pixel step at W // 2)."""
    d = torch.rand(B, 1, H, W, generator=_gen(B, H, W, seed, 1)) * 20
    d[..., W // 2:] += 20
    return d


def coords_and_delta(B, H, W, seed=0):
    """coords1 = x - disparity, and an update of a pixel or two."""
    xs = torch.arange(W, dtype=torch.float32).view(1, 1, 1, W)
    return (xs - disparity(B, H, W, seed)).contiguous(), torch.randn(B, 1, H, W, generator=_gen(B, H, W, seed, 2)) * 1.5


def gradient(B, H, W, seed=0):
    return torch.randn(B, 2, H, W, generator=_gen(B, H, W, seed, 3))


def logits(B, C, H, W, seed=0):
    """Softmax logits over groups of 9 channels: row 0 scaled by 50 (a saturated softmax), one pixel with all logits equal."""
    l = torch.randn(B, C, H, W, generator=_gen(B, C, H, W, seed, 4)) * 2
    l[:, :, 0] *= 50
    l[B - 1, :, H - 1, W // 2] = 0.75
    return l


def hidden(B, C, H, W, seed=0):
    """What the pooling / resize glue carries in the model: GRU hidden states, tanh-bounded."""
    return torch.tanh(torch.randn(B, C, H, W, generator=_gen(B, C, H, W, seed, 5)))


def resize_target(H, W):
    """The loop's up-steps double a grid, or double it less one when the finer grid is odd (update.py:122-124)."""
    return 2 * H, max(2 * W - 1, 1)


def tap_planes(B, ntile, nout, H, W, seed=0):
    return torch.randn(B, ntile, 9 * nout, H, W, generator=_gen(B, ntile, nout, H, W, seed, 6)) * 0.1


# S16 InstanceNorm: the plane is cut into cdiv(HW, 2560) slices of cdiv(HW, slices) pixels (the last one shorter), row-major
IN_PLANES = [(7, 9), (40, 64), (13, 197), (43, 61), (71, 73), (64, 80)]
IN_SLICE_MAX = 2560


def in_slices(HW):
    """-> the slice lengths the S16 InstanceNorm merges."""
    nsl = -(-HW // IN_SLICE_MAX)
    px = -(-HW // nsl)
    return [min(HW, (i + 1) * px) - i * px for i in range(nsl)]


def ramped_planes(B, C, H, W, ramp=8.0, sigma=1.0, offset=0.0, seed=0):
    """Noise of `sigma` plus a vertical ramp of end-to-end height `ramp` (alternating sign per channel) plus `offset`: with the ramp
    the slice means differ by more than the spread inside a slice."""
    x = torch.randn(B, C, H, W, generator=_gen(B, C, H, W, seed, 7)) * sigma + offset
    r = torch.linspace(-0.5, 0.5, H).view(1, 1, H, 1) * ramp if H > 1 else torch.zeros(1, 1, 1, 1)
    sign = torch.tensor([1.0, -1.0]).repeat((C + 1) // 2)[:C].view(1, C, 1, 1)
    return x + r * sign


def between_slice_share(x):
    """min over (b, c) of the share of the plane's biased variance that lies BETWEEN the slice means:
    sum_i n_i (mean_i - mean)^2 / sum (x - mean)^2 — the term Chan's merge adds as d*d*n*f."""
    x = f64(x)
    B, C, H, W = x.shape
    flat = x.reshape(B, C, H * W)
    mean = flat.mean(-1, keepdim=True)
    total = ((flat - mean) ** 2).sum(-1)
    between, lo = 0, 0
    for n in in_slices(H * W):
        between = between + n * (flat[..., lo:lo + n].mean(-1) - mean[..., 0]) ** 2
        lo += n
    return float((between / total).min())
