"""The opt-in deterministic mode on the host side (no GPU): the ordered splat's C ABI (symbols, ABI version, workspace queries, argument
checks), the model's `hip_deterministic` setting, and the host float32 restatement of the documented summation order
(include/tcs_mi355.h, "Ordered splat") that tests/test_gpu_deterministic.py holds the kernels to bit for bit."""
import os
import re
from argparse import Namespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tcs_warp_ordered_workspace_bytes", "tcs_warp_forward_ordered", "tcs_softsplat_ordered_workspace_bytes",
               "tcs_softsplat_sum_ordered")


# ------------------------------------------------------------------------------------------------
# host restatement of the ordered splat
# ------------------------------------------------------------------------------------------------
def splat_entries(flow, valid=None):
    """The contributions of one batch element (flow [2,H,W] float32, valid [H,W] or None) as the kernels form them: arrays (target,
    source, weight), sorted by target and, within a target, by ascending source pixel.  Landing positions and corner weights are
    computed in float32 with one rounding per operation, exactly as k_splat does."""
    flow = np.asarray(flow, dtype=np.float32)
    H, W = flow.shape[1:]
    y, x = np.mgrid[0:H, 0:W]
    with np.errstate(invalid="ignore", over="ignore"):
        fx = (x.astype(np.float32) + flow[0]).ravel()
        fy = (y.astype(np.float32) + flow[1]).ravel()
        ok = np.isfinite(fx) & np.isfinite(fy)
        if valid is not None:
            ok &= np.asarray(valid).ravel() != 0
        x0f, y0f = np.floor(np.where(ok, fx, 0)), np.floor(np.where(ok, fy, 0))
        ok &= (x0f >= -2) & (x0f <= W) & (y0f >= -2) & (y0f <= H)
    src = np.nonzero(ok)[0]
    fx, fy, x0f, y0f = fx[src], fy[src], x0f[src].astype(np.float32), y0f[src].astype(np.float32)
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    X1, Y1 = (x0 + 1).astype(np.float32), (y0 + 1).astype(np.float32)
    w = [(X1 - fx) * (Y1 - fy), (fx - x0f) * (Y1 - fy), (X1 - fx) * (fy - y0f), (fx - x0f) * (fy - y0f)]
    ts, ss, ws = [], [], []
    for k, (dx, dy) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        tx, ty = x0 + dx, y0 + dy
        inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
        ts.append((ty * W + tx)[inside])
        ss.append(src[inside])
        ws.append(w[k][inside].astype(np.float32))
    t, s, wt = np.concatenate(ts), np.concatenate(ss), np.concatenate(ws)
    order = np.lexsort((s, t))
    return t[order], s[order], wt[order]


def splat_sum_ordered(inp, flow, valid=None, scale=None, dtype=np.float32):
    """The ordered splat of inp [B,C,H,W] along flow [B,2,H,W]: per target and channel acc = 0; acc = acc + v * w over the
    contributions in ascending source order, every operation rounded to `dtype` (float32: the kernels' result bit for bit; float64:
    the same order at higher precision).  v = inp, or inp * scale (per source, [B,1,H,W]; the warp's exp(metric), product rounded
    to `dtype`).  Returns [B,C,H,W] of `dtype`."""
    inp = np.asarray(inp, dtype=np.float32)
    B, C, H, W = inp.shape
    out = np.zeros((B, C, H * W), dtype=dtype)
    for b in range(B):
        t, s, w = splat_entries(np.asarray(flow)[b], None if valid is None else np.asarray(valid)[b, 0])
        if t.size == 0:
            continue
        v = inp[b].reshape(C, H * W)[:, s].astype(dtype)
        if scale is not None:
            v = (v * np.asarray(scale)[b, 0].ravel()[s].astype(dtype)).astype(dtype)
        term = (v * w.astype(dtype)).astype(dtype)
        first = np.searchsorted(t, t, side="left")
        rank = np.arange(t.size) - first                    # position within the target's list
        by_rank = np.argsort(rank, kind="stable")
        bounds = np.concatenate([[0], np.cumsum(np.bincount(rank))])
        for r in range(len(bounds) - 1):
            sel = by_rank[bounds[r]:bounds[r + 1]]          # one entry per target at rank r
            out[b][:, t[sel]] = (out[b][:, t[sel]] + term[:, sel]).astype(dtype)
    return out.reshape(B, C, H, W)


def scatter_f64(inp, flow):
    """Order-free float64 reference: np.add.at of inp * w (weights and landing positions as the kernels compute them), and the
    sum of |inp * w| per target (the scale of the fp32 rounding bound)."""
    inp = np.asarray(inp, dtype=np.float64)
    B, C, H, W = inp.shape
    ref, mag, cnt = np.zeros((B, C, H * W)), np.zeros((B, C, H * W)), np.zeros((B, H * W), dtype=np.int64)
    for b in range(B):
        t, s, w = splat_entries(np.asarray(flow)[b])
        term = inp[b].reshape(C, H * W)[:, s] * w.astype(np.float64)
        for c in range(C):
            np.add.at(ref[b, c], t, term[c])
            np.add.at(mag[b, c], t, np.abs(term[c]))
        np.add.at(cnt[b], t, 1)
    return ref.reshape(B, C, H, W), mag.reshape(B, C, H, W), cnt.reshape(B, 1, H, W)


def edge_flow(B, H, W, seed):
    """Random flows plus the edge cases of the splat's rules: NaN, +-Inf, 1e30, and landing positions at -2, -1, W-1, H-1
    (and half a pixel beside them), where corners are clipped."""
    g = np.random.default_rng(seed)
    flow = (g.standard_normal((B, 2, H, W)) * 2.5).astype(np.float32)
    flow[0, 0, 0, 0] = np.nan
    flow[0, 1, 1, 2] = np.inf
    flow[B - 1, 0, 2, 1] = -np.inf
    flow[B - 1, 1, 0, 3] = np.float32(1e30)
    flow[0, 0, 3, 3] = np.float32(-1e30)
    y, x = 2, 4
    for i, (fx, fy) in enumerate(((-2.0, 1.0), (-1.0, 2.0), (W - 1.0, 1.0), (1.0, H - 1.0), (-1.5, -1.5), (W - 0.5, H - 0.5),
                                  (-2.0, -2.0), (W - 1.0, H - 1.0), (float(W), 0.5), (0.5, float(H)))):
        yy, xx = (y + i) % H, (x + 2 * i) % W
        flow[i % B, 0, yy, xx] = np.float32(fx) - np.float32(xx)
        flow[i % B, 1, yy, xx] = np.float32(fy) - np.float32(yy)
    return flow


# ------------------------------------------------------------------------------------------------
# C ABI
# ------------------------------------------------------------------------------------------------
def _lib():
    from tcs_mi355 import native
    return native, native.lib()


def test_abi_version_and_new_symbols():
    native, lib = _lib()
    assert lib.tcs_abi_version() >= 9
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tcs_mi355.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in native.SIGNATURES, name
        assert hasattr(lib, name), name


def test_workspace_queries():
    _, lib = _lib()
    for B, H, W in ((1, 120, 160), (2, 7, 9), (3, 1, 1)):
        s = lib.tcs_softsplat_ordered_workspace_bytes(B, H, W)
        w = lib.tcs_warp_ordered_workspace_bytes(B, 256, H, W)
        assert s > 0 and w > s
        assert s % 256 == 0 and w % 256 == 0
        # the index holds 4 entries per source pixel (int4 unsorted + int2 sorted) and four int / float arrays per pixel
        assert s >= B * H * W * (4 * 16 + 4 * 8 + 3 * 4)
        assert lib.tcs_warp_ordered_workspace_bytes(B, 1, H, W) == w          # no [B, C+2, H, W] accumulator
        assert lib.tcs_softsplat_ordered_workspace_bytes(B + 1, H, W) >= s + (H * W * 96 // 256) * 256
        assert lib.tcs_softsplat_ordered_workspace_bytes(B, H + 1, W) >= s + (B * W * 96 // 256) * 256
    # at the model's shape the ordered warp needs less than the atomic path (its 20 MB accumulator is gone)
    assert lib.tcs_warp_ordered_workspace_bytes(1, 256, 120, 160) < lib.tcs_warp_workspace_bytes(1, 256, 120, 160)
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, -3, 4)):
        assert lib.tcs_softsplat_ordered_workspace_bytes(*bad) == 0, bad
        assert lib.tcs_warp_ordered_workspace_bytes(bad[0], 8, bad[1], bad[2]) == 0, bad
    assert lib.tcs_warp_ordered_workspace_bytes(1, -1, 4, 4) == 0


def test_argument_checks_before_any_launch():
    """TCS_EINVAL on null or out-of-range arguments, as the atomic entry points (the pointers below are never dereferenced)."""
    _, lib = _lib()
    P = 0x1000
    ok = dict(inp=P, flow=P, B=1, C=4, H=8, W=8, out=P, ws=P)

    def sum_call(**kw):
        a = {**ok, **kw}
        return lib.tcs_softsplat_sum_ordered(a["inp"], a["flow"], a["B"], a["C"], a["H"], a["W"], a["out"], a["ws"], None)

    for kw in (dict(inp=None), dict(flow=None), dict(out=None), dict(ws=None), dict(B=0), dict(B=65536), dict(C=0), dict(H=0), dict(W=-1),
               dict(H=30000, W=30000)):
        assert sum_call(**kw) == -1, kw

    def warp_call(**kw):
        a = dict(prev_disp=P, prev_fmap=P, T=P, K=P, Ki=P, base=P, B=1, C=8, H=8, W=8, od=P, of=None, om=P, cur=None, oc=None, ws=P)
        a.update(kw)
        return lib.tcs_warp_forward_ordered(a["prev_disp"], a["prev_fmap"], a["T"], a["K"], a["Ki"], a["base"], a["B"], a["C"], a["H"],
                                            a["W"], a["od"], a["of"], a["om"], a["cur"], a["oc"], a["ws"], None)

    for kw in (dict(prev_disp=None), dict(prev_fmap=None), dict(T=None), dict(K=None), dict(Ki=None), dict(base=None), dict(od=None),
               dict(om=None), dict(ws=None), dict(cur=P), dict(oc=P), dict(B=0), dict(B=65536), dict(C=0), dict(H=0), dict(W=0),
               dict(H=30000, W=30000)):
        assert warp_call(**kw) == -1, kw


# ------------------------------------------------------------------------------------------------
# the model setting
# ------------------------------------------------------------------------------------------------
def _args(**over):
    a = dict(hidden_dims=[128] * 3, shared_backbone=True, corr_levels=4, corr_radius=4, n_downsample=2, context_norm="none",
             slow_fast_gru=False, n_gru_layers=3, mixed_precision=False, init_thres=0.5)
    a.update(over)
    return Namespace(**a)


def test_model_reports_its_deterministic_setting():
    from core.tc_stereo import TCStereo
    assert TCStereo(_args()).hip_deterministic is False
    assert TCStereo(_args(hip_deterministic=False)).hip_deterministic is False
    m = TCStereo(_args(hip_deterministic=True))
    assert m.hip_deterministic is True and m.hip_precision == "fp32"
    with pytest.raises(AttributeError):
        m.hip_deterministic = False                   # fixed at construction
    both = TCStereo(_args(hip_deterministic=True, hip_precision="fp16"))
    assert both.hip_deterministic is True and both.hip_precision == "fp16"
    for bad in (1, 0, "True", None, np.bool_(True)):
        with pytest.raises(ValueError):
            TCStereo(_args(hip_deterministic=bad))


# ------------------------------------------------------------------------------------------------
# the restatement itself
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,H,W,seed", [(2, 5, 7, 9, 0), (1, 3, 33, 45, 1), (2, 4, 16, 24, 2)])
def test_restatement_matches_float64_scatter(B, C, H, W, seed):
    """The float32 restatement of the documented order agrees with an order-free float64 scatter to the fp32 reassociation bound
    (n + 1) * 2^-24 * sum |terms| per target, n = the target's contribution count; and in float64 the same order agrees to 1e-12."""
    g = np.random.default_rng(seed + 100)
    inp = g.standard_normal((B, C, H, W)).astype(np.float32) * 10
    flow = edge_flow(B, H, W, seed)
    got = splat_sum_ordered(inp, flow)
    assert got.dtype == np.float32
    ref, mag, cnt = scatter_f64(inp, flow)
    tol = (cnt + 1) * 2.0 ** -24 * mag
    assert np.all(np.abs(got - ref) <= tol), float(np.max(np.abs(got - ref) - tol))
    assert np.allclose(splat_sum_ordered(inp, flow, dtype=np.float64), ref, rtol=0, atol=1e-12 * max(1.0, float(mag.max())))
    assert cnt.max() >= 4 and (cnt == 0).any()          # overlapping lists and holes both occur


def test_restatement_single_target_and_order():
    """Every source into one target pixel: one list of H*W entries.  The restatement sums it in ascending source order (checked
    against an explicit loop), within the bound of the float64 sum."""
    B, C, H, W = 1, 2, 6, 7
    g = np.random.default_rng(7)
    inp = g.standard_normal((B, C, H, W)).astype(np.float32)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    flow = np.stack([np.float32(3.25) - x, np.float32(2.5) - y])[None].astype(np.float32)
    got = splat_sum_ordered(inp, flow)
    t, s, w = splat_entries(flow[0])
    assert np.array_equal(np.unique(t), [2 * W + 3, 2 * W + 4, 3 * W + 3, 3 * W + 4])
    tgt = 2 * W + 3
    sel = t == tgt
    assert np.array_equal(s[sel], np.arange(H * W))
    for c in range(C):
        acc = np.float32(0)
        for src, wt in zip(s[sel], w[sel]):
            acc = np.float32(acc + np.float32(inp[0, c].ravel()[src] * wt))
        assert got[0, c].ravel()[tgt] == acc
    ref, mag, cnt = scatter_f64(inp, flow)
    assert np.all(np.abs(got - ref) <= (cnt + 1) * 2.0 ** -24 * mag)
