"""The opt-in fp16 precision mode on the host side (no GPU): the `products` field of both convolution descriptors, the model's
`hip_precision` setting, the ABI version, and the register budgets of the single-product kernel instances."""
import ctypes as C
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from tcs_mi355 import native
    return native, native.lib()


def test_descriptors_end_with_products():
    """`products` is the LAST field of tcs_conv_desc and tcs_conv_s16_desc (ABI 8), and a zero-filled descriptor carries 0 there."""
    native, _ = _lib()
    for st in (native.ConvDesc, native.ConvS16Desc):
        assert st._fields_[-1] == ("products", C.c_int), st
        assert st().products == 0
        assert C.sizeof(st) == st.products.offset + C.sizeof(C.c_int) + (-(st.products.offset + 4) % C.alignment(st))
    with open(os.path.join(ROOT, "include", "tcs_mi355.h")) as f:
        hdr = f.read()
    for name in ("tcs_conv_desc", "tcs_conv_s16_desc"):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        fields = re.findall(r"^\s*[\w\s\*]+?[\s\*](\w+)(?:\[\d+\])?;", re.sub(r"/\*.*?\*/", "", body, flags=re.S), re.M)
        assert fields[-1] == "products", (name, fields[-3:])


def test_abi_version_is_at_least_8():
    _, lib = _lib()
    assert lib.tcs_abi_version() >= 8


def _s16_desc(native, cin, cout, k, H, W, products, tile_cfg):
    """A descriptor that is only planned, never launched (tcs_conv2d_s16_group_fused): the pointers are never dereferenced."""
    d = native.ConvS16Desc()
    g = (cin + 15) // 16 * 2
    d.src[0], d.src_ch[0], d.src_groups[0], d.n_src = 0x1000, cin, g, 1
    d.weight = 0x2000
    d.B, d.H, d.W, d.Cin, d.Cout, d.ksize, d.stride = 1, H, W, cin, cout, k, 1
    d.post_scale, d.weight_unscale = 1.0, 1.0
    d.out16, d.out16_groups = 0x3000, (cout + 15) // 16 * 2
    d.tile_cfg, d.products = tile_cfg, products
    return d


def test_zero_filled_products_means_three_and_pairs_need_equal_counts():
    """tcs_conv2d_s16_group_fused plans without launching: a pair of the loop's tile instances fuses when both descriptors say 0 or 3
    (the same contraction), and when both say 1; a 1-product beside a 3-product layer does not (two launches).  Any other count is refused."""
    native, lib = _lib()

    def fused(pa, pb):
        a = _s16_desc(native, 192, 96, 3, 11, 40, pa, 101812)
        b = _s16_desc(native, 27, 96, 1, 11, 40, pb, 101422)
        arr = (C.POINTER(native.ConvS16Desc) * 2)(C.pointer(a), C.pointer(b))
        return lib.tcs_conv2d_s16_group_fused(arr, 2)

    assert fused(0, 0) == 1 and fused(3, 3) == 1 and fused(0, 3) == 1 and fused(3, 0) == 1
    assert fused(1, 1) == 1
    assert fused(1, 0) == 0 and fused(0, 1) == 0 and fused(1, 3) == 0
    assert fused(2, 2) == 0 and fused(-1, -1) == 0


def test_conv_desc_products_is_checked_before_any_launch():
    """tcs_conv2d: products 1 needs TCS_MATH_F16X3; 2 / -1 are TCS_EINVAL (refused before anything is launched)."""
    native, lib = _lib()
    for math, products in ((0, 1), (1, 2), (1, -1), (0, 7)):
        d = native.ConvDesc()
        d.src[0], d.src_ch[0], d.n_src, d.weight, d.out = 0x1000, 16, 1, 0x2000, 0x3000
        d.B, d.H, d.W, d.Cin, d.Cout, d.ksize, d.post_scale = 1, 8, 8, 16, 32, 3, 1.0
        d.out_ctot, d.math, d.weight_unscale, d.products = 32, math, 1.0, products
        assert lib.tcs_conv2d(C.byref(d), None) == -1, (math, products)


def _args(**over):
    from argparse import Namespace
    a = dict(hidden_dims=[128] * 3, shared_backbone=True, corr_levels=4, corr_radius=4, n_downsample=2, context_norm="none",
             slow_fast_gru=False, n_gru_layers=3, mixed_precision=False, init_thres=0.5)
    a.update(over)
    return Namespace(**a)


def test_model_reports_its_precision():
    from core.tc_stereo import TCStereo
    assert TCStereo(_args()).hip_precision == "fp32"
    assert TCStereo(_args(hip_precision="fp32")).hip_precision == "fp32"
    m = TCStereo(_args(hip_precision="fp16"))
    assert m.hip_precision == "fp16"
    with pytest.raises(AttributeError):
        m.hip_precision = "fp32"                      # fixed at construction
    # mixed_precision keeps its no-op meaning
    assert TCStereo(_args(mixed_precision=True)).hip_precision == "fp32"
    for bad in ("bf16", "fp64", "FP16", None):
        with pytest.raises(ValueError):
            TCStereo(_args(hip_precision=bad))


def test_precision_is_per_model_instance():
    """Two models in one process: each layer's packing reads its own model's setting; the exempt layers stay 3-product in both."""
    from core.tc_stereo import TCStereo
    from core.update import products_of
    a, b = TCStereo(_args(hip_precision="fp16")), TCStereo(_args())
    assert products_of(a.update_block.gru08.convzr) == 1 and products_of(b.update_block.gru08.convzr) == 0
    assert products_of(a.disp_grad_refine.conv_4_4[0]) == 1 and products_of(a.context_zqr_convs[0]) == 1
    for m in (a, b):
        assert products_of(m.hiddenstate_update.convzr) == 0 and products_of(m.hiddenstate_update.convs[2]) == 0
        assert products_of(m.update_block.flow_head.conv2) == 0 and products_of(m.disp_grad_refine.residual_head[2]) == 0


def test_single_product_kernel_register_budgets():
    """The k_conv_s16_x1 instances (tcs_conv_s16_desc.products = 1) hold the budgets of their 3-product counterparts
    (tests/test_host.py::test_kernel_register_budgets): no spills; one-row 32-channel LINEAR <= 96 VGPRs, GRU_ZR <= 104, GRU_Q and tap
    partials <= 128; pair kernels <= 96."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    if not os.path.exists(f"{kr.LLVM}/clang-offload-bundler") or not os.path.exists(f"{kr.LLVM}/llvm-readelf"):
        pytest.skip("LLVM binary utilities not found")
    native, _ = _lib()
    res = kr.kernel_resources(native.lib_path())
    names = sorted(res)
    nice = dict(zip(names, kr.demangle(names)))
    x1 = [k for k in names if nice[k].startswith(("void k_conv_s16_x1", "void k_conv_f16x1"))]
    spilled = [nice[k] for k in x1 if res[k].get("vgpr_spill_count", 0)]
    assert not spilled, spilled
    seen = {"linear": 0, "gru_zr": 0, "gru_q": 0, "taps": 0}
    for k in names:
        m = re.match(r"void k_conv_s16_x1<(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (true|false)>", nice[k])
        if not m:
            continue
        ks, mt, rows, kst, nst, stride, epi, rs, rpw = (int(v) for v in m.groups()[:9])
        v = res[k]["vgpr_count"]
        if mt != 1 or rpw != 1:
            continue
        if m.group(10) == "true":
            assert v <= 128, (nice[k], v)
            seen["taps"] += 1
        elif epi == 0:
            assert v <= 96, (nice[k], v)
            seen["linear"] += 1
        elif epi == 1:
            assert v <= 104, (nice[k], v)
            seen["gru_zr"] += 1
        elif epi == 2:
            assert v <= 128, (nice[k], v)
            seen["gru_q"] += 1
    assert all(n > 0 for n in seen.values()), seen
    pairs = [k for k in names if nice[k].startswith("void k_conv_s16_x1_pair<")]
    assert len(pairs) >= 3, [nice[k] for k in pairs]
    for k in pairs:
        assert res[k]["vgpr_count"] <= 96, (nice[k], res[k]["vgpr_count"])
    assert any(nice[k].startswith("void k_conv_f16x1<") for k in names) and any(nice[k].startswith("void k_conv_f16x1_ws<") for k in names)
