"""The tile instances of tcs_conv2d_s16 (csrc/tcs_conv_s16.hip, launch_s16_cfg) that the library is meant to offer — ONE table,
read by the host test that compares it with the library's planner (test_s16_instances_host.py: what plans with TCS_OK equals this
table, both ways) and by the GPU tests that run every row of it against fp64 (test_gpu_s16_instances.py, and the tile loops of
test_gpu_s16.py / test_gpu_precision.py).  A tile added to or removed from the library changes this table first.

A tile code is RS*10000 + MT*1000 + ROWS*100 + KSTEPS*10 + NSTAGE (RS: 0 plain, 1 row split, 2 two rows per wave; MT: 32-channel cout
tiles per workgroup; ROWS: output rows per workgroup; KSTEPS: 16-channel k-steps per stage; NSTAGE: LDS stages), optionally + 100000 *
CSPLIT (block -> XCD mapping, not a template parameter: every code runs with every CSPLIT digit).
"""
import ctypes as C

EPI_LINEAR, EPI_GRU_ZR, EPI_GRU_Q, EPI_DECONV2X, EPI_BLEND9 = 0, 1, 2, 3, 4
EPI_NAME = {EPI_LINEAR: "linear", EPI_GRU_ZR: "gru_zr", EPI_GRU_Q: "gru_q", EPI_DECONV2X: "deconv2x", EPI_BLEND9: "blend9"}
TCS_OK, TCS_EINVAL, TCS_EUNSUPPORTED = 0, -1, -3

_PLAIN_3x3 = (1411, 2411, 1811, 1412, 1413, 2412, 2413, 1512, 2512, 1812, 2812, 11000 + 1412, 11000 + 1413)     # the last two: 12412, 12413 (row split)
_RPW2_3x3 = (21812, 22812, 21412, 21411, 22412)
_ALL_1x1 = (1412, 2412, 1422, 1423, 2422, 2423, 1442, 2442)

# (ksize, stride, epilogue, taps) -> tile codes
TABLE = {
    (3, 1, EPI_LINEAR, 0): _PLAIN_3x3 + _RPW2_3x3,
    (3, 1, EPI_LINEAR, 1): (1411, 1412, 1812, 21812),          # with tap partials: their own instances
    (3, 1, EPI_GRU_ZR, 0): _PLAIN_3x3 + _RPW2_3x3,
    (3, 1, EPI_GRU_Q, 0): _PLAIN_3x3 + _RPW2_3x3,
    (3, 1, EPI_DECONV2X, 0): _PLAIN_3x3,
    (3, 2, EPI_LINEAR, 0): (1412, 1411),
    (1, 2, EPI_LINEAR, 0): (1412, 1422),
    (1, 1, EPI_LINEAR, 0): _ALL_1x1,
    (1, 1, EPI_GRU_ZR, 0): _ALL_1x1,
    (1, 1, EPI_GRU_Q, 0): _ALL_1x1,
    (1, 1, EPI_BLEND9, 0): (1412, 1422, 1423, 1442),           # 9 outputs = one 32-channel tile: no MT = 2
}
KINDS = sorted(TABLE)
PRODUCTS = (3, 1)


def digits(code):
    """Tile code -> (row_split, rows_per_wave, mt, rows, ksteps, nstage) as tcs_s16_instance reports them."""
    c = code % 100000
    rs = c // 10000
    return (1 if rs == 1 else 0, 2 if rs == 2 else 1, (c // 1000) % 10, (c // 100) % 10, (c // 10) % 10, c % 10)


def all_instances():
    """Every (ksize, stride, epilogue, taps, code) of the table, in a fixed order."""
    return [k + (code,) for k in KINDS for code in TABLE[k]]


def tiles(ksize, stride, epilogue, taps=0, mt=None):
    """The table's codes of one kind (optionally only those with `mt` cout tiles per workgroup)."""
    return [c for c in TABLE[(ksize, stride, epilogue, taps)] if mt is None or digits(c)[2] == mt]


def linear_tiles(ksize, stride, cins, cout, csplit_too=False):
    """The LINEAR codes of the table that a layer with these sources and outputs can run: 64-channel tiles (MT = 2) need an even number
    of 32-channel tiles, KSTEPS k-steps per stage must divide every source's k-steps.  `csplit_too`: each code also with CSPLIT = 1."""
    out = []
    for code in TABLE[(ksize, stride, EPI_LINEAR, 0)]:
        _, _, mt, _, kst, _ = digits(code)
        if ((cout + 31) // 32) % mt == 0 and all(((c + 15) // 16) % kst == 0 for c in cins):
            out += [code, 100000 + code] if csplit_too else [code]
    return out


def inst_id(inst):
    k, s, e, t, code = inst
    return f"{k}x{k}s{s}-{EPI_NAME[e]}{'-taps' if t else ''}-{code}"


def code_space():
    """The whole space the host test sweeps: RS 0..2, MT 1..2, ROWS 4 / 5 / 8, KSTEPS 1 / 2 / 4, NSTAGE 1..3."""
    return [rs * 10000 + mt * 1000 + rows * 100 + kst * 10 + nst
            for rs in (0, 1, 2) for mt in (1, 2) for rows in (4, 5, 8) for kst in (1, 2, 4) for nst in (1, 2, 3)]


def plan(native, lib, d):
    """(return code, native.S16Instance) of tcs_conv2d_s16_plan for descriptor `d`."""
    out = native.S16Instance()
    rc = lib.tcs_conv2d_s16_plan(C.byref(d), C.byref(out))
    return rc, out


def instance_key(p):
    """What identifies a kernel instance in a tcs_s16_instance: the hashable the model-coverage test compares."""
    return (p.ksize, p.stride, p.epilogue, p.taps, p.products, p.row_split, p.rows_per_wave, p.mt, p.rows, p.ksteps, p.nstage)


def table_keys():
    """instance_key() of every table row times PRODUCTS."""
    out = set()
    for (k, s, e, t, code) in all_instances():
        rs, rpw, mt, rows, kst, nst = digits(code)
        for pr in PRODUCTS:
            out.add((k, s, e, t, pr, rs, rpw, mt, rows, kst, nst))
    return out


def host_desc(native, ksize, stride, epilogue, taps, cins, cout, H, W, B=1, products=0, tile_cfg=0):
    """A descriptor that is only planned (tcs_conv2d_s16_plan): like `_s16_desc` of test_precision_host.py, with the operands each
    epilogue insists on.  The pointers are made up and never dereferenced."""
    d = native.ConvS16Desc()
    for i, c in enumerate(cins):
        d.src[i], d.src_ch[i], d.src_groups[i] = 0x1000 * (i + 1), c, (c + 15) // 16 * 2
    d.n_src = len(cins)
    d.weight = 0x20000
    d.B, d.H, d.W, d.Cin, d.Cout, d.ksize, d.stride = B, H, W, sum(cins), cout, ksize, stride
    d.post_scale, d.weight_unscale = 1.0, 1.0
    d.epilogue, d.tile_cfg, d.products = epilogue, tile_cfg, products
    if taps:                # asked of every epilogue: only 3x3 stride-1 LINEAR launches may carry tap partials
        d.tap_weights, d.tap_out, d.tap_nout, d.tap_tiles, d.tap_unscale = 0x40000, 0x50000, 1, (cout + 31) // 32, 1.0
    if epilogue == EPI_LINEAR:
        d.out16, d.out16_groups = 0x30000, (cout + 15) // 16 * 2
    elif epilogue == EPI_GRU_ZR:
        hid = cout // 2
        d.h, d.h_groups, d.out16, d.out16_groups, d.out32, d.out_ctot = 0x60000, hid // 8, 0x30000, hid // 8, 0x70000, hid
    elif epilogue == EPI_GRU_Q:
        d.h, d.h_groups, d.z, d.out16, d.out16_groups = 0x60000, cout // 8, 0x70000, 0x30000, cout // 8
    elif epilogue == EPI_DECONV2X:
        d.out16, d.out16_groups = 0x30000, (cout // 4 + 15) // 16 * 2
    elif epilogue == EPI_BLEND9:
        d.blend_cand, d.blend_cand_ctot, d.blend_refined = 0x80000, 9, 0x90000
    return d


# The refinement loop's layers at the BASELINE shapes: (name, ksize, stride, epilogue, taps, cins, cout, scale divisor of the image).
# Sizes from core/update.py (gru08: 128 hidden + 128 motion + 128 from gru16; gru16's launches after the K split; the gradient
# predictor's conv_4_8 and up-blocks; a Lightfuse-like 1x1 gate; DispRefine's w_head[2]).
LOOP_LAYERS = [
    ("gru08.zr", 3, 1, EPI_GRU_ZR, 0, (128, 128, 128), 256, 4),
    ("gru08.q", 3, 1, EPI_GRU_Q, 0, (128, 128, 128), 128, 4),
    ("gru16.zr", 3, 1, EPI_GRU_ZR, 0, (128,), 256, 8),
    ("gru16.q", 3, 1, EPI_GRU_Q, 0, (128, 128), 128, 8),
    ("gru32.zr", 3, 1, EPI_GRU_ZR, 0, (128, 128), 256, 16),
    ("gru32.q", 3, 1, EPI_GRU_Q, 0, (128, 128), 128, 16),
    ("conv_4_8", 3, 2, EPI_LINEAR, 0, (64,), 96, 4),
    ("gate1x1", 1, 1, EPI_LINEAR, 0, (128, 64), 256, 4),
    ("w_head2", 1, 1, EPI_BLEND9, 0, (128,), 9, 4),
    ("up_16_8", 3, 1, EPI_DECONV2X, 0, (128,), 4 * 96, 16),
    ("up_8_4", 3, 1, EPI_DECONV2X, 0, (96,), 4 * 64, 8),
]
IMAGES = ((480, 640), (384, 1248))          # 640x480 and the KITTI shape: 1/4 scale = 120x160 and 96x312
BATCHES = (1, 4, 8)


def layer_grid(image, div):
    return image[0] // div, image[1] // div
