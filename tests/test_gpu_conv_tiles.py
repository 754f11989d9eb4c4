"""Every tile instance of the fp32-tensor convolution (tcs_conv2d) against fp64, at the shapes where it runs.

tcs_conv2d picks its tile from the grid size alone (launch_by_tile in csrc/tcs_conv.hip, launch_f16_tile in
csrc/tcs_conv_f16.hip), and no caller can force one.  So this module restates both heuristics (`f32_tile`, `f16x3_tile`),
gives every case the tile it is meant to reach, checks that the mirror agrees, and checks at import time that the cases reach
every tile the mirror can return: a heuristic change that leaves a tile untested fails here.  The references are fp64
PyTorch on the CPU, at the bars of test_gpu_parity.py::test_conv2d_vs_torch (<= 2e-5 for He-scaled weights).

Also here: the GRU epilogues on the fp32-tensor path, the grouped launches of ops.grouped (tcs_conv2d_group), the lifetime of
the tensors a grouped block records, and both branches of tcs_instance_norm."""
import pytest
import torch
import torch.nn.functional as F

from conftest import maxdiff

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from tcs_mi355 import native
    native.lib()
    return torch.device("cuda:0")


def D(x, dev):
    return x.to(dev).contiguous()


def cdiv(a, b):
    return -(-a // b)


# ---- tile mirrors -----------------------------------------------------------------------------------------------------
F32_TILES = {"mfma<3,1,16>", "mfma<3,2,8>", "mfma<3,4,8>", "mfma<1,1,32>", "mfma<1,2,32>", "mfma<1,4,32>"}
F16X3_TILES = {"f16x3<3,MT=1>", "f16x3<3,MT=2>", "f16x3<3,MT=1,ROWS=5>", "f16x3_ws<3,NP=4>", "f16x3_ws<3,NP=8>",
               "f16x3<1,MT=1>", "f16x3<1,MT=2>", "f16x3<3,STRIDE=2>"}


def f32_tile(B, H, W, Cout, k):
    """k_conv_mfma<KS, MT, KC> that tcs_conv2d launches (Cin > 1, 1x1 / 3x3): cout_tile (tcs_conv_common.h) and
    launch_by_tile (tcs_conv.hip): the widest cout tile that still gives >= 512 blocks, KC = 8 / 16 (3x3 wide / narrow), 32 (1x1)."""
    nt = 128 if Cout > 64 else (64 if Cout > 32 else 32)
    cout_pad = cdiv(Cout, nt) * nt
    npatch = cdiv(W, 32) * cdiv(H, 4)
    while nt > 32 and npatch * B * (cout_pad // nt) < 512:
        nt >>= 1
    mt = nt // 32
    kc = 32 if k == 1 else (8 if mt > 1 else 16)
    name = f"mfma<{k},{mt},{kc}>"
    assert name in F32_TILES, name
    return name


def f16x3_tile(B, H, W, Cout, k, stride=1):
    """k_conv_f16x3 / k_conv_f16x3_ws instance that tcs_conv2d launches for fp16-split weights: launch_f16_any / launch_f16_tile
    (tcs_conv_f16.hip).  MT = 2 when it still gives >= 512 blocks; 3x3: 5-row patches when they balance the grid better (MT = 1,
    400 < blocks <= 768), the wave-specialised kernel with 8 / 4 producer waves for <= 200 / <= 400 blocks."""
    if stride == 2:
        name = "f16x3<3,STRIDE=2>"
        assert k == 3
        return name
    nct32 = cdiv(Cout, 32)
    npx = cdiv(W, 32)
    px_tiles = npx * cdiv(H, 4) * B
    mt = 2 if (nct32 % 2 == 0 and px_tiles * (nct32 // 2) >= 512) else 1
    if k == 1:
        name = f"f16x3<1,MT={mt}>"
    else:
        wg4 = npx * cdiv(H, 4) * B * (nct32 // mt)
        wg5 = npx * cdiv(H, 5) * B * (nct32 // mt)
        e4 = wg4 / (256.0 * ((wg4 + 255) // 256))
        e5 = wg5 / (256.0 * ((wg5 + 255) // 256))
        blocks_mt1 = px_tiles * nct32
        if mt == 1 and e5 > e4 + 0.05 and 400 < wg4 <= 768:
            name = "f16x3<3,MT=1,ROWS=5>"
        elif blocks_mt1 <= 200:
            name = "f16x3_ws<3,NP=8>"
        elif blocks_mt1 <= 400:
            name = "f16x3_ws<3,NP=4>"
        else:
            name = f"f16x3<3,MT={mt}>"
    assert name in F16X3_TILES, name
    return name


def tile_of(math, B, H, W, cout, k, stride=1):
    return f32_tile(B, H, W, cout, k) if math == "f32" else f16x3_tile(B, H, W, cout, k, stride)


# ---- cases: (id, math, ksize, stride, B, source channels, Cout, H, W, tile meant to be hit) --------------------------------------
CONV_CASES = [
    # source boundaries off the multiples of 8: KC = 8 chunks of the fp32 kernel and the 8-channel groups of the fp16-split loader straddle
    # them (the per-channel source select instead of the src_align8 one)
    ("f32-3x3-mt4", "f32", 3, 1, 1, (27, 14), 127, 237, 317, "mfma<3,4,8>"),       # partial 128 tile; a KC = 8 chunk straddles 27 | 14
    ("f32-3x3-mt2", "f32", 3, 1, 4, (19, 13), 64, 120, 160, "mfma<3,2,8>"),        # the batched leg's candidate stem (32 -> 64)
    ("f32-3x3-mt1", "f32", 3, 1, 1, (20, 12, 9), 40, 13, 45, "mfma<3,1,16>"),
    ("f32-1x1-mt4", "f32", 1, 1, 2, (20, 16), 200, 120, 160, "mfma<1,4,32>"),
    ("f32-1x1-mt2", "f32", 1, 1, 4, (36,), 64, 118, 157, "mfma<1,2,32>"),
    ("f32-1x1-mt1", "f32", 1, 1, 1, (9, 7, 11, 5), 96, 11, 70, "mfma<1,1,32>"),
    ("f16-3x3-mt2", "f16x3", 3, 1, 1, (61, 43), 256, 117, 157, "f16x3<3,MT=2>"),
    ("f16-3x3-mt1", "f16x3", 3, 1, 1, (45, 51), 96, 120, 160, "f16x3<3,MT=1>"),
    ("f16-3x3-rows5", "f16x3", 3, 1, 1, (77, 51), 128, 120, 160, "f16x3<3,MT=1,ROWS=5>"),
    ("f16-3x3-ws4", "f16x3", 3, 1, 1, (37, 27), 64, 120, 160, "f16x3_ws<3,NP=4>"),
    ("f16-3x3-ws8", "f16x3", 3, 1, 1, (24, 19), 72, 21, 75, "f16x3_ws<3,NP=8>"),
    ("f16-1x1-mt2", "f16x3", 1, 1, 1, (61, 39), 256, 120, 160, "f16x3<1,MT=2>"),
    ("f16-1x1-mt1", "f16x3", 1, 1, 1, (27,), 96, 17, 45, "f16x3<1,MT=1>"),
    ("f16-3x3-s2", "f16x3", 3, 2, 1, (37, 27), 96, 61, 83, "f16x3<3,STRIDE=2>"),
]

# ConvGRU at hidden `hid`: convzr reads cat(h, x) (2*hid outputs), convq cat(r*h, x) (hid outputs), update.py:81-85
# (id, B, hid, x channels, H, W, {math: (ZR tile, Q tile)}); x is split off the multiples of 8 (sources h | x0 | x1 ...)
GRU_CASES = [
    ("gru08", 1, 128, (61, 67, 128), 120, 160, {"f32": ("mfma<3,2,8>", "mfma<3,1,16>"),
                                              "f16x3": ("f16x3<3,MT=2>", "f16x3<3,MT=1,ROWS=5>")}),
    ("hid96-b2", 2, 96, (19, 21), 120, 160, {"f32": ("mfma<3,4,8>", "mfma<3,2,8>"),            # z | r boundary inside a 128 tile
                                          "f16x3": ("f16x3<3,MT=2>", "f16x3<3,MT=1>")}),
    ("hid96-b4", 4, 96, (19, 21), 117, 157, {"f32": ("mfma<3,4,8>", "mfma<3,4,8>"),
                                          "f16x3": ("f16x3<3,MT=2>", "f16x3<3,MT=1>")}),
    ("hid48-small", 1, 48, (11, 13), 13, 45, {"f32": ("mfma<3,1,16>", "mfma<3,1,16>"),
                                           "f16x3": ("f16x3_ws<3,NP=8>", "f16x3_ws<3,NP=8>")}),
]


def _check_case_lists_cover_every_tile():
    seen = {"f32": set(), "f16x3": set()}
    for _, math, k, stride, B, cins, cout, H, W, tile in CONV_CASES:
        assert tile_of(math, B, H, W, cout, k, stride) == tile, (math, k, B, cout, H, W, tile)
        seen[math].add(tile)
    assert seen["f32"] == F32_TILES, F32_TILES - seen["f32"]
    assert seen["f16x3"] == F16X3_TILES, F16X3_TILES - seen["f16x3"]
    gru_seen = set()
    for _, B, hid, xs, H, W, tiles in GRU_CASES:
        for math, (zr, q) in tiles.items():
            assert tile_of(math, B, H, W, 2 * hid, 3) == zr and tile_of(math, B, H, W, hid, 3) == q, (math, hid, B, H, W)
        gru_seen |= {("zr", tiles["f32"][0]), ("q", tiles["f32"][1])}
    f32_3x3 = {t for t in F32_TILES if t.startswith("mfma<3,")}
    assert gru_seen == {(e, t) for e in ("zr", "q") for t in f32_3x3}, gru_seen


_check_case_lists_cover_every_tile()          # at import: fails collection loudly when a heuristic change strands a tile


def test_tile_mirrors_reach_the_loop_layers():
    """Layers of the loop at 640x480 (1/4 scale: 120x160), through the mirrors (pure host arithmetic)."""
    assert f32_tile(4, 120, 160, 64, 3) == "mfma<3,2,8>"              # DispGradPredictor.conv_grad_candidate_stem[0], 4 sequences
    assert f32_tile(1, 120, 160, 64, 3) == "mfma<3,1,16>"             # ... one sequence: the grouped pair's instance
    assert f32_tile(1, 120, 160, 32, 3) == "mfma<3,1,16>"             # conv_grad_stem[0]
    assert f16x3_tile(1, 120, 160, 128, 3) == "f16x3<3,MT=1,ROWS=5>"  # 128 -> 128 at 640x480 / 4
    assert f16x3_tile(1, 120, 160, 256, 3) == "f16x3<3,MT=2>"
    assert f16x3_tile(1, 120, 160, 64, 3) == "f16x3_ws<3,NP=4>"


# ---- per tile, against fp64 ----------------------------------------------------------------------------------------------
def _he(gen, cout, cin, k):
    return torch.randn(cout, cin, k, k, generator=gen) * (2.0 / (cin * k * k)) ** 0.5


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_tile_vs_fp64(dev, case):
    from tcs_mi355 import ops, s16
    name, math, k, stride, B, cins, cout, H, W, tile = case
    gen = torch.Generator().manual_seed(sum(cins) * 1000 + cout + k)
    cin = sum(cins)
    w = _he(gen, cout, cin, k)
    b = torch.randn(cout, generator=gen) * 0.1
    xs = [torch.randn(B, c, H, W, generator=gen) for c in cins]
    ref = F.conv2d(torch.cat(xs, 1).double(), w.double(), b.double(), stride=stride, padding=k // 2)
    Ho, Wo = ref.shape[2:]
    add = torch.randn(B, cout, Ho, Wo, generator=gen)
    pc = ops.pack_conv(D(w, dev), D(b, dev), math)
    assert pc.math == (ops.MATH_F16X3 if math == "f16x3" else ops.MATH_F32)
    xd = [D(x, dev) for x in xs]
    add_d, add64 = D(add, dev), add.double()
    tol = 2e-5

    def conv(**kw):
        return ops.conv2d(pc, xd, stride=stride, **kw)

    assert maxdiff(conv(), ref) <= tol, "linear + bias"
    acts = (("relu", torch.relu, 0.25), ("leaky", lambda t: F.leaky_relu(t, 0.01), 0.5),
            ("sigmoid", torch.sigmoid, 0.75), ("tanh", torch.tanh, 2.0))
    for act, fn, scale in acts:
        assert maxdiff(conv(act=act, post_scale=scale), scale * fn(ref)) <= tol, act
    assert maxdiff(conv(addend=add_d), ref + add64) <= tol, "addend"
    assert maxdiff(conv(act="relu_add_relu", addend=add_d), torch.relu(torch.relu(ref) + add64)) <= tol, "relu_add_relu"

    # into channels [coff, coff + cout) of a wider buffer: every other channel keeps its sentinel, bit for bit
    coff, ctot = 13, cout + 13 + 21
    wide = torch.randn(B, ctot, Ho, Wo, generator=gen).to(dev)
    before = wide.clone()
    conv(act="leaky", addend=add_d, out=wide, out_coff=coff)
    assert maxdiff(wide[:, coff:coff + cout], F.leaky_relu(ref + add64, 0.01)) <= tol, "out_coff"
    assert torch.equal(wide[:, :coff], before[:, :coff]) and torch.equal(wide[:, coff + cout:], before[:, coff + cout:]), "out_coff sentinel"

    if stride == 1:
        # S16 output at a nonzero group offset: the groups before and after, the border and the channels of a partly written group
        # keep their contents bit for bit
        goff, G = 2, s16.groups_for(cout) + 4
        o16 = s16.S16(torch.randn(B, G, 2, Ho + 2, Wo + 2, 8, generator=gen).half().to(dev), cout)
        before = o16.data.clone()
        ops.conv2d(pc, xd, act="relu", addend=add_d, out16=o16, out16_group_offset=goff)
        assert maxdiff(s16.from_s16(o16, cout, group_offset=goff), torch.relu(ref + add64)) <= tol, "out16"
        untouched = torch.ones(before.shape, dtype=torch.bool, device=dev)
        for c in range(cout):
            untouched[:, goff + c // 8, :, 1:-1, 1:-1, c % 8] = False
        assert torch.equal(o16.data[untouched], before[untouched]), "out16 sentinel"


# ---- GRU epilogues on the fp32-tensor path ---------------------------------------------------------------------------------
@pytest.mark.parametrize("math", ["f32", "f16x3"])
@pytest.mark.parametrize("case", GRU_CASES, ids=[c[0] for c in GRU_CASES])
def test_gru_epilogues_vs_fp64(dev, case, math):
    """ops.gru_gates / ops.gru_update against an fp64 ConvGRU (update.py:81-85, 30-34): with and without the context addends,
    keep_z both ways, and the state update in place (out=h)."""
    from tcs_mi355 import ops
    name, B, hid, xch, H, W, _ = case
    gen = torch.Generator().manual_seed(hid * 7 + B)
    cin = hid + sum(xch)
    wzr, wq = _he(gen, 2 * hid, cin, 3), _he(gen, hid, cin, 3)
    bzr, bq = torch.randn(2 * hid, generator=gen) * 0.1, torch.randn(hid, generator=gen) * 0.1
    h = torch.tanh(torch.randn(B, hid, H, W, generator=gen))
    xs = [torch.randn(B, c, H, W, generator=gen) for c in xch]
    cz, cr, cq = (torch.randn(B, hid, H, W, generator=gen) for _ in range(3))
    pzr = ops.pack_conv(D(wzr, dev), D(bzr, dev), math)
    pq = ops.pack_conv(D(wq, dev), D(bq, dev), math)
    hd, xd = D(h, dev), [D(x, dev) for x in xs]
    tol = 2e-5

    zr = F.conv2d(torch.cat([h] + xs, 1).double(), wzr.double(), bzr.double(), padding=1)
    for with_add in (True, False):
        z, rh = ops.gru_gates(pzr, [hd] + xd, hd, cz=D(cz, dev) if with_add else None, cr=D(cr, dev) if with_add else None)
        az, ar = (cz.double(), cr.double()) if with_add else (0.0, 0.0)
        assert maxdiff(z, torch.sigmoid(zr[:, :hid] + az)) <= tol, ("z", with_add)
        assert maxdiff(rh, torch.sigmoid(zr[:, hid:] + ar) * h.double()) <= tol, ("rh", with_add)

    # the candidate reads cat(r*h, x) as the kernel produced it, so that only the update launch is measured
    qpre = F.conv2d(torch.cat([rh.cpu()] + xs, 1).double(), wq.double(), bq.double(), padding=1)
    z64, h64 = z.cpu().double(), h.double()
    for keep_z, with_add in ((False, True), (True, False), (True, True), (False, False)):
        q = torch.tanh(qpre + (cq.double() if with_add else 0.0))
        want = z64 * h64 + (1 - z64) * q if keep_z else (1 - z64) * h64 + z64 * q
        got = ops.gru_update(pq, [rh] + xd, hd, z, cq=D(cq, dev) if with_add else None, keep_z=keep_z)
        assert maxdiff(got, want) <= tol, (keep_z, with_add)
        h_io = hd.clone()
        ops.gru_update(pq, [rh] + xd, h_io, z, cq=D(cq, dev) if with_add else None, keep_z=keep_z, out=h_io)
        assert torch.equal(h_io, got), ("in place", keep_z, with_add)


# ---- ops.grouped / tcs_conv2d_group ----------------------------------------------------------------------------------------
def _layer(gen, dev, cin, cout, H, W, B=1, math="f32"):
    from tcs_mi355 import ops
    x = torch.randn(B, cin, H, W, generator=gen)
    w, b = _he(gen, cout, cin, 3), torch.randn(cout, generator=gen) * 0.1
    return x, w, b, ops.pack_conv(D(w, dev), D(b, dev), math)


@pytest.mark.parametrize("pair, fused", [
    (dict(a=(2, 32, 1, "f32"), b=(32, 64, 1, "f32"), H=120, W=160), True),       # DispGradPredictor's stems, first layers, C2 size
    (dict(a=(2, 32, 1, "f32"), b=(32, 64, 1, "f32"), H=61, W=83), True),         # ... at a ragged size
    (dict(a=(2, 32, 4, "f32"), b=(32, 64, 4, "f32"), H=120, W=160), False),      # the batched leg: 32 -> 64 takes MT = 2, key mismatch
    (dict(a=(2, 32, 2, "f32"), b=(32, 64, 1, "f32"), H=29, W=45), False),        # batch sizes differ
    (dict(a=(32, 32, 1, "f16x3"), b=(2, 32, 1, "f32"), H=61, W=83), False),      # fp16-split first: launched while planning, order reverses
    (dict(a=(2, 32, 1, "f32"), b=(32, 48, 1, "f16x3"), H=61, W=83), False),      # fp16-split second
], ids=["c2", "ragged", "batched-leg", "batch-mismatch", "f16-first", "f16-second"])
def test_grouped_conv_launch_equals_separate_launches(dev, pair, fused):
    """ops.grouped: bit-equal to the separate launches and within 2e-5 of fp64, with S16 outputs (as the loop uses them) and with fp32
    outputs; `report` tells one launch from two without launching anything."""
    from tcs_mi355 import ops, s16
    gen = torch.Generator().manual_seed(5)
    H, W = pair["H"], pair["W"]
    la, lb = pair["a"], pair["b"]
    xa, wa, ba, pca = _layer(gen, dev, la[0], la[1], H, W, la[2], la[3])
    xb, wb, bb, pcb = _layer(gen, dev, lb[0], lb[1], H, W, lb[2], lb[3])
    xad, xbd = D(xa, dev), D(xb, dev)
    assert pca.math == (ops.MATH_F32 if la[3] == "f32" else ops.MATH_F16X3)
    ra = torch.relu(F.conv2d(xa.double(), wa.double(), ba.double(), padding=1))
    rb = torch.relu(F.conv2d(xb.double(), wb.double(), bb.double(), padding=1))

    # fp32 outputs
    sep_a, sep_b = ops.conv2d(pca, [xad], act="relu"), ops.conv2d(pcb, [xbd], act="relu")
    with ops.grouped(report=True) as g:
        grp_a = ops.conv2d(pca, [xad], act="relu")
        grp_b = ops.conv2d(pcb, [xbd], act="relu")
    assert g.fused == [fused]
    assert torch.equal(grp_a, sep_a) and torch.equal(grp_b, sep_b)
    assert maxdiff(grp_a, ra) <= 2e-5 and maxdiff(grp_b, rb) <= 2e-5

    # S16 outputs
    def outs():
        return s16.zeros(la[2], la[1], H, W, dev), s16.zeros(lb[2], lb[1], H, W, dev)
    sa, sb = outs()
    ops.conv2d(pca, [xad], act="relu", out16=sa)
    ops.conv2d(pcb, [xbd], act="relu", out16=sb)
    ga, gb = outs()
    with ops.grouped(report=True) as g:
        ops.conv2d(pca, [xad], act="relu", out16=ga)
        ops.conv2d(pcb, [xbd], act="relu", out16=gb)
    assert g.fused == [fused]
    assert torch.equal(ga.data, sa.data) and torch.equal(gb.data, sb.data)
    assert maxdiff(ga.float(), ra) <= 2e-5 and maxdiff(gb.float(), rb) <= 2e-5


# ---- lifetime of what a grouped block records ------------------------------------------------------------------------------
def test_grouped_block_keeps_temporary_sources_alive(dev):
    """A recorded descriptor holds raw pointers.  Sources made inline (`x.contiguous()` of a non-contiguous view) are temporaries: the
    block must keep them until its launch at __exit__, or a later same-size temporary of the block may take over their memory."""
    from tcs_mi355 import ops
    gen = torch.Generator().manual_seed(6)
    H, W = 61, 83
    xa, _, _, pca = _layer(gen, dev, 32, 32, H, W)
    xb, _, _, pcb = _layer(gen, dev, 32, 64, H, W)
    ta, tb = D(xa, dev).transpose(2, 3).contiguous(), D(xb, dev).transpose(2, 3).contiguous()     # [B, C, W, H] storage
    sep_a = ops.conv2d(pca, [ta.transpose(2, 3).contiguous()], act="relu")
    sep_b = ops.conv2d(pcb, [tb.transpose(2, 3).contiguous()], act="relu")
    with ops.grouped():
        grp_a = ops.conv2d(pca, [ta.transpose(2, 3).contiguous()], act="relu")
        grp_b = ops.conv2d(pcb, [tb.transpose(2, 3).contiguous()], act="relu")
    assert torch.equal(grp_a, sep_a) and torch.equal(grp_b, sep_b)
    # the same through S16 outputs and fp32 addends
    from tcs_mi355 import s16
    add = D(torch.randn(1, 32, W, H, generator=gen), dev)
    ea, eb = s16.zeros(1, 32, H, W, dev), s16.zeros(1, 64, H, W, dev)
    ops.conv2d(pca, [ta.transpose(2, 3).contiguous()], addend=add.transpose(2, 3).contiguous(), out16=ea)
    ops.conv2d(pcb, [tb.transpose(2, 3).contiguous()], out16=eb)
    ga, gb = s16.zeros(1, 32, H, W, dev), s16.zeros(1, 64, H, W, dev)
    with ops.grouped():
        ops.conv2d(pca, [ta.transpose(2, 3).contiguous()], addend=add.transpose(2, 3).contiguous(), out16=ga)
        ops.conv2d(pcb, [tb.transpose(2, 3).contiguous()], out16=gb)
    assert torch.equal(ga.data, ea.data) and torch.equal(gb.data, eb.data)


def test_s16_grouped_block_keeps_temporary_addends_alive(dev):
    from tcs_mi355 import ops, s16
    gen = torch.Generator().manual_seed(7)
    H, W = 29, 45
    x = D(torch.randn(1, 64, H, W, generator=gen), dev)
    x16 = s16.to_s16(x)
    pca = ops.pack_conv(D(_he(gen, 64, 64, 3), dev), None, "f16x3")
    pcb = ops.pack_conv(D(_he(gen, 64, 64, 3), dev), None, "f16x3")
    aa = D(torch.randn(1, 64, H, W, generator=gen), dev).transpose(2, 3).contiguous()          # [B, C, W, H] storage
    ab = D(torch.randn(1, 64, H, W, generator=gen), dev).transpose(2, 3).contiguous()
    sep_a, _ = s16.conv2d(pca, [x16], act="relu", addend=aa.transpose(2, 3).contiguous(), tile_cfg=101412)
    sep_b, _ = s16.conv2d(pcb, [x16], act="relu", addend=ab.transpose(2, 3).contiguous(), tile_cfg=101412)
    with s16.grouped(report=True) as g:
        grp_a, _ = s16.conv2d(pca, [x16], act="relu", addend=aa.transpose(2, 3).contiguous(), tile_cfg=101412)
        grp_b, _ = s16.conv2d(pcb, [x16], act="relu", addend=ab.transpose(2, 3).contiguous(), tile_cfg=101412)
    assert g.fused == [True]
    assert torch.equal(grp_a.data, sep_a.data) and torch.equal(grp_b.data, sep_b.data)


def test_grad_predictor_with_non_contiguous_inputs(dev):
    """DispGradPredictor.forward(g5=..., cands=...) accepts non-contiguous inputs (the public fp32 API; g5 used to reach the residual
    head's addend as a non-contiguous tensor and raise) and gives bit for bit the result of the same call with contiguous copies.
    forward makes its own contiguous copies up front, so this does not exercise the grouped blocks' lifetimes: the two tests above do."""
    from argparse import Namespace
    from core.update import DispGradPredictor
    from tcs_mi355 import ops
    torch.manual_seed(8)
    m = DispGradPredictor(Namespace()).to(dev).eval()
    gen = torch.Generator().manual_seed(9)
    B, H, W = 1, 32, 48
    g5 = D(torch.randn(B, 2, W, H, generator=gen), dev).transpose(2, 3)                # non-contiguous views
    disp = D(torch.rand(B, 1, H, W, generator=gen) * 20, dev)
    cands = ops.grad_candidates(disp).transpose(2, 3).contiguous().transpose(2, 3)
    assert not g5.is_contiguous() and not cands.is_contiguous()
    clist = [D(torch.randn(B, 64, H >> i, W >> i, generator=gen), dev) for i in range(3)]
    with torch.no_grad():
        ref_g, ref_c = m(None, disp, clist, g5=g5.contiguous(), cands=cands.contiguous())
        ref_g, ref_c = ref_g.clone(), ref_c.clone()
        g, c = m(None, disp, clist, g5=g5, cands=cands)
    assert torch.equal(g, ref_g) and torch.equal(c, ref_c)


# ---- tcs_instance_norm: cached (<= 32768 pixels) and re-reading branches ---------------------------------------------------
@pytest.mark.parametrize("B, C_, H, W", [(1, 3, 128, 256), (1, 3, 129, 256), (2, 3, 480, 640)],
                         ids=["hw32768-cached", "hw33024-uncached", "480x640-b2"])
def test_instance_norm_both_branches_vs_fp64(dev, B, C_, H, W):
    """Against fp64 F.instance_norm, no worse than 4x PyTorch CPU fp32's own error on the same input.  Plane 0 sits at a large offset
    with a small spread (the two-pass variance must hold), plane 1 is plain randn, the last plane is constant (variance 0: the output is exactly 0 plus the
    addend; the constant 100 sums exactly in fp32, so the mean is exact)."""
    from tcs_mi355 import ops
    gen = torch.Generator().manual_seed(H + W + B)
    x = torch.randn(B, C_, H, W, generator=gen)
    x[:, 0] = 100.0 + 0.01 * x[:, 0]
    x[:, -1] = 100.0
    add = torch.randn(B, C_, H, W, generator=gen)
    xd, addd = D(x, dev), D(add, dev)
    acts = {"none": lambda t: t, "relu": torch.relu, "leaky": lambda t: F.leaky_relu(t, 0.01)}
    n64 = F.instance_norm(x.double(), eps=1e-5)
    n32 = F.instance_norm(x, eps=1e-5)
    for act, fn in acts.items():
        for with_add in (False, True):
            a64 = add.double() if with_add else 0.0
            ref = fn(n64) + a64
            cpu = fn(n32) + (add if with_add else 0.0)
            got = ops.instance_norm(xd, act=act, addend=addd if with_add else None)
            for c in range(C_ - 1):
                e_cpu, e_hip = maxdiff(cpu[:, c], ref[:, c]), maxdiff(got[:, c], ref[:, c])
                assert e_hip <= 4 * e_cpu, (act, with_add, c, e_hip, e_cpu)
            want = add[:, -1] if with_add else torch.zeros(B, H, W)
            assert torch.equal(got[:, -1].cpu(), want), (act, with_add, "constant plane")
