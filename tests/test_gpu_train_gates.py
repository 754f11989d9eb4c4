"""tcs_mi355.train_ops.gru_reset / gru_update on the MI355X: every output and gradient against the float64 restatement of
test_train_gates_host.py under the project's rule e_hip <= 4 e_ref + one float32 ulp of the tensor's largest magnitude, per tensor
and case, nothing excluded (e_ref: the error of the reference's own float32 values in tests/golden/train_gates.npz for the chained
cells, or, for inputs the golden file does not hold, of the same restatement in float32 on the GPU); chunk / split views read in
place; alignment and tails of both the 16-byte and the 4-byte path; the loop's shapes; saturated gates; partial gradients; what the
nodes save; determinism, double backward, the no-grad path, half-precision inputs; and a trainer-shaped step through the patched
cells.  Every comparison prints e_ref, e_hip and the ulp floor before it asserts; no MI355X run of this module has been recorded
yet, so no figures are quoted here."""
import numpy as np
import pytest
import torch

from test_train_gates_host import (CELLS, KEEPS, case_tensors, golden, grad_keys, reset_restate, restate, run_cell, update_restate)

pytestmark = pytest.mark.gpu


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
    print(f"{tag}: max|x| {top:.3e} e_ref {e_ref:.3e} e_hip {e_hip:.3e} floor {floor:.3e}")
    assert e_hip <= 4 * e_ref + floor, (tag, e_hip, e_ref, floor)


def random_inputs(dev, B, C, H, W, seed=5, spread=2.0):
    """z_pre / r_pre as chunk views of one [B,2C,H,W] tensor, cz / cr / cq as split views of one [B,3C,H,W] tensor."""
    g = torch.Generator().manual_seed(seed)
    zr = (spread * torch.randn(B, 2 * C, H, W, generator=g)).to(dev)
    ctx = torch.randn(B, 3 * C, H, W, generator=g).to(dev)
    t = {"q_pre": (spread * torch.randn(B, C, H, W, generator=g)).to(dev), "h": (2 * torch.rand(B, C, H, W, generator=g) - 1).to(dev),
         "g": torch.randn(B, C, H, W, generator=g).to(dev)}
    t["z_pre"], t["r_pre"] = zr.chunk(2, dim=1)
    t["cz"], t["cr"], t["cq"] = ctx.split(C, dim=1)
    return t


RESET_IN, UPDATE_IN = ("r_pre", "h", "cr"), ("z_pre", "q_pre", "h", "cz", "cq")


def op_results(t, reset, update, keep, dtype=None, device=None):
    """Both ops separately on the tensors of `t` (None context terms allowed), each with upstream t['g']: outputs and gradients."""
    def leaf(k):
        x = t.get(k)
        if x is None:
            return None
        x = x.detach() if dtype is None else x.detach().to(device=device, dtype=dtype)
        return x.requires_grad_(True)
    g = t["g"] if dtype is None else t["g"].to(device=device, dtype=dtype)
    out = {}
    for names, op, value, tag in ((RESET_IN, reset, "rh", "reset d"),
                                  (UPDATE_IN, lambda *a: update(*a, z_keeps_h=keep), "h_new", "update d")):
        L = [leaf(k) for k in names]
        y = op(*L)
        out[value] = y.detach()
        have = [(k, x) for k, x in zip(names, L) if x is not None]
        for (k, _), d in zip(have, torch.autograd.grad(y, [x for _, x in have], g)):
            out[tag + k] = d
    return out


def check_ops(tag, t, keep):
    """Both ops on `t` under the rule: float64 on the CPU, e_ref from the restatement in float32 where `t` lives."""
    from tcs_mi355 import train_ops as to
    hip = op_results(t, to.gru_reset, to.gru_update, keep)
    r32 = op_results(t, reset_restate, update_restate, keep)
    r64 = op_results(t, reset_restate, update_restate, keep, torch.float64, "cpu")
    assert set(hip) == set(r64)
    for k in sorted(r64):
        assert hip[k].dtype == torch.float32 and hip[k].is_contiguous(), k
        compare(f"{tag} keep={int(keep)} {k}", hip[k], r64[k], r32[k])
    return hip


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("i", range(5))
def test_golden_cases(dev, gold, cell, i):
    """The chained cell against the reference's own values and gradients, and each op alone on the same inputs."""
    from tcs_mi355 import train_ops as to
    t = case_tensors(gold, cell, i, device=dev)
    r64 = restate(cell, case_tensors(gold, cell, i, torch.float64))
    hip = run_cell(cell, t, to.gru_reset, to.gru_update)
    for key in ("h_new",) + grad_keys(cell):
        compare(f"{cell} c{i} chained {key}", hip[key], r64[key], torch.from_numpy(gold[f"{cell}_c{i}_{key}"]))
    z_pre, r_pre = t["zr"].chunk(2, dim=1)
    sep = {"z_pre": z_pre, "r_pre": r_pre, "q_pre": t["q0"], "h": t["h"], "g": t["g"], "cz": t.get("cz"), "cr": t.get("cr"), "cq": t.get("cq")}
    check_ops(f"{cell} c{i} alone", sep, KEEPS[cell])


def test_chunk_and_split_views_are_read_in_place(dev):
    from tcs_mi355 import train_ops as to
    B, C, H, W = 2, 4, 6, 11
    t = random_inputs(dev, B, C, H, W, seed=6)
    assert not any(t[k].is_contiguous() for k in ("z_pre", "r_pre", "cz", "cr", "cq"))
    c = {k: v.contiguous() for k, v in t.items()}
    for keep in (False, True):
        a, b = op_results(t, to.gru_reset, to.gru_update, keep), op_results(c, to.gru_reset, to.gru_update, keep)
        for k in a:
            assert torch.equal(a[k], b[k]), k
    out_bytes = -(-B * C * H * W * 4 // 512) * 512          # the allocator's 512-byte blocks
    with torch.no_grad():
        for fn in (lambda: to.gru_reset(t["r_pre"], t["h"], t["cr"]),
                   lambda: to.gru_update(t["z_pre"], t["q_pre"], t["h"], t["cz"], t["cq"], z_keeps_h=False)):
            fn()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = fn()
            torch.cuda.synchronize()
            rise = torch.cuda.max_memory_allocated() - base
            print(f"forward on views: peak {rise} bytes over the baseline, the output is {out_bytes}")
            assert rise == out_bytes and out.is_contiguous()


def padded(x, pad):
    """A copy of x [B,C,H,W] whose batch stride is C*H*W + pad elements."""
    B, n = x.shape[0], x[0].numel()
    buf = torch.zeros(B, n + pad, device=x.device)
    buf[:, :n] = x.reshape(B, n)
    v = buf[:, :n].view(x.shape)
    assert v.stride(0) == n + pad and v.data_ptr() == buf.data_ptr()
    return v


@pytest.mark.parametrize("B,C,H,W,pad,keep", [
    (2, 3, 5, 7, 0, False),        # H*W = 35: planes and batch elements start 4-byte aligned only (4-byte path)
    (2, 2, 6, 6, 4, True),         # H*W = 36, batch stride 76 floats = 19 x 16 bytes: odd in 16-byte units (16-byte path)
    (2, 2, 6, 6, 1, False),        # the same through a batch stride of 73 floats: no multiple of 16 bytes (4-byte path)
    (2, 1, 1, 1023, 0, True),      # one less and one more than four blocks of the 4-byte path (256 elements a block)
    (2, 1, 1, 1025, 0, False),
    (2, 1, 4, 255, 0, False),      # 1020 and 1028: one 16-byte unit less and more than a block of the 16-byte path (1024 elements)
    (2, 1, 4, 257, 0, True),
    (3, 2, 32, 32, 0, False),      # exactly two full blocks per batch element
])
def test_alignment_and_tails(dev, B, C, H, W, pad, keep):
    t = random_inputs(dev, B, C, H, W, seed=7)
    if pad:
        t = {k: (padded(v, pad) if k != "g" else v) for k, v in t.items()}
        assert all(t[k].stride(0) == C * H * W + pad for k in t if k != "g")
    check_ops(f"{B}x{C}x{H}x{W} pad {pad}", t, keep)


@pytest.mark.parametrize("B,C,H,W,keep", [(2, 128, 80, 180, False), (2, 128, 10, 23, False), (2, 128, 10, 23, True)])
def test_loop_shapes(dev, B, C, H, W, keep):
    check_ops(f"{B}x{C}x{H}x{W}", random_inputs(dev, B, C, H, W, seed=8), keep)


def test_saturated_gates(dev):
    """|pre| = 100: finite outputs and gradients, gate gradients zero or of the order of exp(-100)."""
    from tcs_mi355 import train_ops as to
    B, C, H, W = 2, 3, 5, 8
    g = torch.Generator().manual_seed(9)
    sign = lambda: (2.0 * (torch.rand(B, C, H, W, generator=g) < 0.5) - 1.0).to(dev)      # noqa: E731
    t = {"z_pre": 100 * sign(), "r_pre": 100 * sign(), "q_pre": 100 * sign(), "h": (2 * torch.rand(B, C, H, W, generator=g) - 1).to(dev),
         "g": torch.randn(B, C, H, W, generator=g).to(dev)}
    for keep in (False, True):
        hip = check_ops("saturated", t, keep)
        for k, v in hip.items():
            assert bool(torch.isfinite(v).all()), k
        for k in ("reset dr_pre", "update dz_pre", "update dq_pre"):
            print(f"saturated keep={int(keep)} {k}: max {float(hip[k].abs().max()):.3e}")
            assert float(hip[k].abs().max()) <= 1e-40, k
        assert bool(((hip["h_new"] == t["h"]) | (hip["h_new"].abs() == 1)).all())


def test_partial_gradients(dev):
    from types import SimpleNamespace

    from tcs_mi355 import train_ops as to
    t = random_inputs(dev, 2, 3, 5, 7, seed=10)
    for keep in (False, True):
        full = op_results(t, to.gru_reset, to.gru_update, keep)
        for op, names, tag in ((to.gru_reset, RESET_IN, "reset d"), (lambda *a: to.gru_update(*a, z_keeps_h=keep), UPDATE_IN, "update d")):
            for k in names:
                L = [t[n].detach().requires_grad_(n == k) for n in names]
                d, = torch.autograd.grad(op(*L), [x for x in L if x.requires_grad], t["g"])
                assert torch.equal(d, full[tag + k]), (tag, k)
    # inside the node a context term's gradient IS its pre-activation's tensor, and what is not needed is None
    with torch.no_grad():
        ctx = SimpleNamespace(saved_tensors=(t["r_pre"], t["h"], t["cr"]), needs_input_grad=(True, False, True))
        d_pre, d_h, d_cr = to._GruReset.backward(ctx, t["g"])
        assert d_cr is d_pre and d_h is None and torch.equal(d_pre, full["reset dr_pre"])
        ctx.needs_input_grad = (False, True, False)
        assert [x is None for x in to._GruReset.backward(ctx, t["g"])] == [True, False, True]
        ctx = SimpleNamespace(saved_tensors=tuple(t[k] for k in UPDATE_IN), z_keeps_h=True, needs_input_grad=(True, True, False, True, True, False))
        d_z, d_q, d_h, d_cz, d_cq, none = to._GruUpdate.backward(ctx, t["g"])
        assert d_cz is d_z and d_cq is d_q and d_h is None and none is None
        assert torch.equal(d_z, full["update dz_pre"]) and torch.equal(d_q, full["update dq_pre"])       # `full` is keep=True here
        ctx.needs_input_grad = (False, False, False, True, False, False)
        assert [x is None for x in to._GruUpdate.backward(ctx, t["g"])] == [True, True, True, False, True, True]
    # through autograd the returned context gradients have the pre-activation's values
    assert torch.equal(full["reset dcr"], full["reset dr_pre"]) and torch.equal(full["update dcz"], full["update dz_pre"])
    assert torch.equal(full["update dcq"], full["update dq_pre"])


def test_no_gradient_buffer_for_what_is_not_needed(dev):
    """Only h requires grad: the backward allocates that one gradient (and reads neither q_pre nor cq)."""
    from tcs_mi355 import train_ops as to
    t = random_inputs(dev, 2, 8, 20, 45, seed=11)
    one = -(-t["h"].numel() * 4 // 512) * 512
    h = t["h"].detach().requires_grad_(True)
    for out in (to.gru_reset(t["r_pre"], h, t["cr"]), to.gru_update(t["z_pre"], t["q_pre"], h, t["cz"], t["cq"], z_keeps_h=False)):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        d, = torch.autograd.grad(out, h, t["g"])
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - base
        print(f"backward for h alone: peak {rise} bytes over the baseline, one gradient is {one}")
        assert rise == one


def test_saved_tensors_share_storage_with_the_inputs(dev):
    from tcs_mi355 import train_ops as to
    t = random_inputs(dev, 2, 3, 5, 8, seed=12)
    L = {k: v.detach().requires_grad_(True) for k, v in t.items() if k != "g"}
    storages = {v.untyped_storage().data_ptr() for v in L.values()}
    saved = []

    def pack(x):
        saved.append(x)
        return x
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda x: x):
        to.gru_reset(L["r_pre"], L["h"], L["cr"])
        n_reset = len(saved)
        to.gru_update(L["z_pre"], L["q_pre"], L["h"], L["cz"], L["cq"], z_keeps_h=True)
    assert n_reset == 3 and len(saved) == 8, [tuple(x.shape) for x in saved]
    assert all(x.untyped_storage().data_ptr() in storages for x in saved)


def test_determinism_double_backward_no_grad_and_half_inputs(dev):
    from tcs_mi355 import train_ops as to
    t = random_inputs(dev, 2, 3, 5, 8, seed=13)
    for keep in (False, True):
        a, b = op_results(t, to.gru_reset, to.gru_update, keep), op_results(t, to.gru_reset, to.gru_update, keep)
        for k in a:
            assert torch.equal(a[k], b[k]), k
        # a non-contiguous upstream gradient is made contiguous
        g_nc = t["g"].transpose(2, 3).contiguous().transpose(2, 3)
        assert not g_nc.is_contiguous()
        c = op_results({**t, "g": g_nc}, to.gru_reset, to.gru_update, keep)
        for k in a:
            assert torch.equal(a[k], c[k]), k
        # no-grad path: no node, the same bits
        with torch.no_grad():
            L = {k: v.detach().requires_grad_(True) for k, v in t.items()}
            rh = to.gru_reset(L["r_pre"], L["h"], L["cr"])
            h_new = to.gru_update(L["z_pre"], L["q_pre"], L["h"], L["cz"], L["cq"], z_keeps_h=keep)
        assert rh.grad_fn is None and h_new.grad_fn is None and not rh.requires_grad and not h_new.requires_grad
        assert torch.equal(rh, a["rh"]) and torch.equal(h_new, a["h_new"])
        plain = to.gru_update(t["z_pre"], t["q_pre"], t["h"], t["cz"], t["cq"], z_keeps_h=keep)       # nothing requires grad
        assert plain.grad_fn is None and torch.equal(plain, a["h_new"])
    # the two conventions differ
    assert not torch.equal(to.gru_update(t["z_pre"], t["q_pre"], t["h"], z_keeps_h=False), to.gru_update(t["z_pre"], t["q_pre"], t["h"], z_keeps_h=True))
    # double backward raises
    x = t["h"].detach().requires_grad_(True)
    d, = torch.autograd.grad(to.gru_reset(t["r_pre"], x), x, t["g"], create_graph=True)
    with pytest.raises(RuntimeError):
        d.sum().backward()
    x = t["q_pre"].detach().requires_grad_(True)
    d, = torch.autograd.grad(to.gru_update(t["z_pre"], x, t["h"], z_keeps_h=True), x, t["g"], create_graph=True)
    with pytest.raises(RuntimeError):
        d.sum().backward()
    # half-precision inputs: float32 outputs, gradients in the input's dtype, equal to the float32 path on the same values
    for half in (torch.float16, torch.bfloat16):
        z16, q16, h16 = (t[k].to(half).requires_grad_(True) for k in ("z_pre", "q_pre", "h"))
        out = to.gru_update(z16, q16, h16, t["cz"], z_keeps_h=False)
        z32, q32, h32 = (x.detach().float().requires_grad_(True) for x in (z16, q16, h16))
        ref = to.gru_update(z32, q32, h32, t["cz"], z_keeps_h=False)
        assert out.dtype == torch.float32 and torch.equal(out, ref)
        for d16, d32, x16 in zip(torch.autograd.grad(out, [z16, q16, h16], t["g"]), torch.autograd.grad(ref, [z32, q32, h32], t["g"]),
                                 (z16, q16, h16)):
            assert d16.dtype == half and d16.shape == x16.shape and torch.equal(d16, d32.to(half))
        r16 = t["r_pre"].to(half).requires_grad_(True)
        rh = to.gru_reset(r16, t["h"])
        assert rh.dtype == torch.float32 and torch.equal(rh, to.gru_reset(r16.detach().float(), t["h"]))
        d16, = torch.autograd.grad(rh, r16, t["g"])
        assert d16.dtype == half


@pytest.mark.parametrize("cell", ["gru", "fuse", "hu"])
def test_trainer_shaped_step(dev, cell):
    """A cell of torch.nn.Conv2d layers with the reference's attribute names (C = 8, Cx = 8), two iterations, a sum loss and
    backward(): once through patch_reference_cells, once as written in the reference in plain PyTorch ops in float32 on the GPU, once
    in float64 on the CPU.  Every parameter and input gradient under the rule, e_ref being the plain formulation's own error."""
    from types import SimpleNamespace

    from tcs_mi355 import train_ops as to
    B, C, Cx, H, W = 2, 8, 8, 12, 20

    class ConvGRU(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.convzr, self.convq = torch.nn.Conv2d(C + Cx, 2 * C, 3, padding=1), torch.nn.Conv2d(C + Cx, C, 3, padding=1)

        def forward(self, h, cz, cr, cq, *x_list):                     # update.py:77-87 without the asserts
            x = torch.cat(x_list, dim=1)
            z, r = self.convzr(torch.cat([h, x], dim=1)).chunk(2, dim=1)
            z, r = torch.sigmoid(z + cz), torch.sigmoid(r + cr)
            q = torch.tanh(self.convq(torch.cat([r * h, x], dim=1)) + cq)
            return (1 - z) * h + z * q

    class Lightfuse(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.convzr, self.convq = torch.nn.Conv2d(C + Cx, 2 * C, 1), torch.nn.Conv2d(C + Cx, C, 1)

        def forward(self, h, x):                                       # update.py:26-36
            z, r = self.convzr(torch.cat([h, x], dim=1)).chunk(2, dim=1)
            z, r = torch.sigmoid(z), torch.sigmoid(r)
            q = torch.tanh(self.convq(torch.cat([r * h, x], dim=1)))
            return z * h + (1 - z) * q

    class HiddenstateUpdater(Lightfuse):
        def __init__(self):
            super().__init__()
            self.convs = torch.nn.Sequential(torch.nn.Conv2d(1, Cx, 1), torch.nn.LeakyReLU(), torch.nn.Conv2d(Cx, Cx, 1))

        def forward(self, h, x):                                       # update.py:57-68
            return Lightfuse.forward(self, h, self.convs(x))
    cls = {"gru": ConvGRU, "fuse": Lightfuse, "hu": HiddenstateUpdater}[cell]
    g = torch.Generator().manual_seed(14)
    data = {"h": 2 * torch.rand(B, C, H, W, generator=g) - 1, "x": torch.randn(B, 1 if cell == "hu" else Cx, H, W, generator=g),
            "ctx": torch.randn(B, 3 * C, H, W, generator=g)}

    def run(mode):
        dtype, d = (torch.float64, torch.device("cpu")) if mode == "f64" else (torch.float32, dev)
        torch.manual_seed(15)
        m = cls().to(d).to(dtype)
        L = {k: v.to(d).to(dtype).clone().requires_grad_(True) for k, v in data.items()}
        undo = to.patch_reference_cells(SimpleNamespace(ConvGRU=ConvGRU, Lightfuse=Lightfuse, HiddenstateUpdater=HiddenstateUpdater)) \
            if mode == "hip" else (lambda: None)
        try:
            h = L["h"]
            for _ in range(2):
                h = m(h, *L["ctx"].split(C, dim=1), L["x"]) if cell == "gru" else m(h, L["x"])
            h.sum().backward()
        finally:
            undo()
        names = [n for n, _ in m.named_parameters()] + sorted(L)
        grads = [p.grad for p in m.parameters()] + [L[k].grad for k in sorted(L)]
        return h.detach(), dict(zip(names, grads))
    (h_hip, g_hip), (h_32, g_32), (h_64, g_64) = run("hip"), run("f32"), run("f64")
    compare(f"trainer step {cell} h", h_hip, h_64, h_32)
    for n in g_64:
        if cell != "gru" and n == "ctx":
            assert g_hip[n] is None and g_64[n] is None
            continue
        assert g_hip[n] is not None and float(g_64[n].abs().max()) > 0, n
        compare(f"trainer step {cell} {n}", g_hip[n], g_64[n], g_32[n])
