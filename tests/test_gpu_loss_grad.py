"""The differentiable training objective on the MI355X (tcs_mi355.train_losses, the tcs_*loss*_bwd kernels of tcs_loss.hip): every
gradient against the fp64 autograd restatement of test_loss_grad_host.py under the rule e_hip <= 4 e_ref + one fp32 ulp of the
tensor's largest gradient, where e_ref is the error of the reference's own float32 gradients (tests/golden/loss_grad.npz; for a
setting the golden file does not hold, of the same restatement in float32) against that restatement; the structure of the
gradients; determinism; the upstream gradient; and the objective inside an autograd chain."""
import numpy as np
import pytest
import torch

from test_loss_grad_host import INPUTS, PART_INPUTS, golden, init_loss_torch, objective_torch, restate_grads
from test_losses_host import case_inputs, targets

pytestmark = pytest.mark.gpu
KEYS = {"up": "flow_predictions", "q": "flow_q_predictions", "grad": "disp_grad_q_predictions", "flow_mono": "flow_mono",
        "flow_init": "flow_init", "cost_volume": "cost_volume"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from tcs_mi355 import native
    native.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    return golden()


def _cases(gold):
    return [(i, [int(v) for v in c]) for i, c in enumerate(gold["cases"])]


class Leaves:
    """A make_loss_case on the device with the six predictions as leaves: the stacked tensors (the lists are views of them, as
    forward(test_mode=False) returns them) or, separate=True, one leaf per list entry (as the reference's model returns them)."""

    def __init__(self, case, dev, iters, separate=False):
        t = {k: torch.from_numpy(v).to(dev) for k, v in case.items()}
        self.flow, self.valid, self.iters, self.separate = t["flow"], t["valid"], iters, separate
        self.single = {n: t[n].clone().requires_grad_(True) for n in ("flow_mono", "flow_init", "cost_volume")}
        if separate:
            self.up = [[t["up"][i, r].clone().requires_grad_(True) for r in range(2)] for i in range(iters)]
            self.q = [[t["q"][i, r].clone().requires_grad_(True) for r in range(2)] for i in range(iters)]
            self.grad = [t["grad"][i].clone().requires_grad_(True) for i in range(iters)]
        else:
            self.stack = {n: t[n].clone().requires_grad_(True) for n in ("up", "q", "grad")}
            self.up = [[self.stack["up"][i, 0], self.stack["up"][i, 1]] for i in range(iters)]
            self.q = [[self.stack["q"][i, 0], self.stack["q"][i, 1]] for i in range(iters)]
            self.grad = [self.stack["grad"][i] for i in range(iters)]
        self.out = {"flow_predictions": self.up, "flow_q_predictions": self.q, "disp_grad_q_predictions": self.grad, **self.single}

    def wrt(self, names=INPUTS):
        """The flat list of leaves behind `names`, for torch.autograd.grad."""
        flat = []
        for n in names:
            if n in self.single:
                flat.append(self.single[n])
            elif not self.separate:
                flat.append(self.stack[n])
            elif n == "grad":
                flat += self.grad
            else:
                flat += [x for pair in getattr(self, n) for x in pair]
        return flat

    def gather(self, names, flat):
        """The gradients of wrt(names), restacked into the layout of the case's arrays."""
        res, flat = {}, list(flat)
        for n in names:
            if n in self.single or not self.separate:
                res[n] = flat.pop(0)
            elif n == "grad":
                res[n] = torch.stack([flat.pop(0) for _ in range(self.iters)])
            else:
                res[n] = torch.stack([torch.stack([flat.pop(0), flat.pop(0)]) for _ in range(self.iters)])
        return res

    def grads(self, loss, names=INPUTS, **kw):
        return self.gather(names, torch.autograd.grad(loss, self.wrt(names), **kw))


def compare(tag, hip, g64, ref32, kink):
    """The issue's rule on one tensor.  Prints the figures before it asserts."""
    hip = hip.detach().cpu().double()
    assert hip.shape == g64.shape, (tag, hip.shape, g64.shape)
    assert bool(torch.isfinite(hip).all()), tag
    keep = ~kink
    assert int(kink.sum()) <= 1e-3 * kink.numel(), (tag, "kinks", int(kink.sum()))
    top = float(g64.abs().max())
    e_ref = float(((ref32.double() - g64).abs() * keep).max())
    e_hip = float(((hip - g64).abs() * keep).max())
    floor = float(np.spacing(np.float32(top)))
    print(f"{tag}: max|g| {top:.3e} e_ref {e_ref:.3e} e_hip {e_hip:.3e} floor {floor:.3e} kinks {int(kink.sum())}")
    assert e_hip <= 4 * e_ref + floor, (tag, e_hip, e_ref, floor)


class Reference:
    """The fp64 restatement and the reference's float32 gradients of one case and setting, computed once."""
    _cache = {}

    @classmethod
    def get(cls, gold, i, c, k, dense):
        key = (i, k, dense)
        if key not in cls._cache:
            case = case_inputs(c)
            g64, info = restate_grads(case, c[4], k, dense)
            on_golden = (k, int(dense)) == (c[5], c[6])
            g32 = None
            ref = {}
            for part in g64:
                for n in g64[part]:
                    name = f"c{i}_{part}_{n}"
                    if on_golden and name in gold:
                        ref[part, n] = torch.from_numpy(gold[name])
                    else:
                        if g32 is None:
                            g32, _ = restate_grads(case, c[4], k, dense, dtype=torch.float32)
                        ref[part, n] = g32[part][n]
            cls._cache[key] = (case, g64, ref, info)
        return cls._cache[key]


SETTINGS = [(1, True), (1, False), (3, True), (3, False)]


@pytest.mark.parametrize("separate", [False, True])
@pytest.mark.parametrize("i", range(5))
def test_training_objective_gradients(dev, gold, i, separate):
    from tcs_mi355 import train_losses as tl
    c = [int(v) for v in gold["cases"][i]]
    for k, dense in SETTINGS:
        case, g64, ref, info = Reference.get(gold, i, c, k, dense)
        L = Leaves(case, dev, c[4], separate)
        total, vec = tl.training_objective(L.out, L.flow, L.valid, init_k=k, dense_gt=dense, sync=False)
        assert total.grad_fn is not None and total.ndim == 0
        got = L.grads(total)
        for n in INPUTS:
            compare(f"objective c{i} k{k} dense{int(dense)} sep{int(separate)} {n}", got[n], g64["total"][n], ref["total", n],
                    info["kinks"][n])


@pytest.mark.parametrize("separate", [False, True])
@pytest.mark.parametrize("i", range(5))
def test_each_loss_alone(dev, gold, i, separate):
    from tcs_mi355 import train_losses as tl
    c = [int(v) for v in gold["cases"][i]]
    w = tl.loss_weights(c[4])
    for k, dense in SETTINGS:
        case, g64, ref, info = Reference.get(gold, i, c, k, dense)
        L = Leaves(case, dev, c[4], separate)
        v, ggt, ngt = tl.gt_targets(L.flow, L.valid)
        losses = {"seq": tl.sequence_loss(L.single["flow_mono"], L.single["flow_init"], L.up, L.flow, v, w)[0],
                  "init": tl.init_loss(L.single["cost_volume"], L.flow, v, k=k, scale=0.25, threshold=0.5)[0],
                  "norm": tl.disp_normal_loss(L.q, ngt, v, w, scale=0.25, dense_gt=dense)[0],
                  "grad": tl.disp_grad_loss(L.grad, ggt, v, w, scale=0.25, dense_gt=dense)[0]}
        for part, loss in losses.items():
            assert loss.grad_fn is not None and loss.ndim == 0, part
            got = L.grads(loss, PART_INPUTS[part])
            for n in PART_INPUTS[part]:
                compare(f"{part} alone c{i} k{k} dense{int(dense)} sep{int(separate)} {n}", got[n], g64[part][n], ref[part, n],
                        info["kinks"][n])


@pytest.mark.parametrize("i", range(5))
def test_structure(dev, gold, i):
    """What holds without a tolerance: zero off the masks, the cost volume's column pattern and sums, the empty case."""
    from tcs_mi355 import train_losses as tl
    c = [int(v) for v in gold["cases"][i]]
    k, dense = c[5], bool(c[6])
    case, g64, ref, info = Reference.get(gold, i, c, k, dense)
    L = Leaves(case, dev, c[4])
    total, _ = tl.training_objective(L.out, L.flow, L.valid, init_k=k, dense_gt=dense, sync=False)
    got = {n: g.cpu() for n, g in L.grads(total).items()}
    v = info["valid"]
    for n in ("up", "flow_mono", "flow_init"):
        assert not got[n][~v.expand_as(got[n])].any(), n
    assert not got["grad"][~info["grad_valid"].expand_as(got["grad"])].any()
    gcv, mask = got["cost_volume"].double(), info["init_mask"]
    nz = (gcv != 0).sum(1, keepdim=True)
    assert int(nz.max()) <= k + 2
    assert not nz[~mask].any()
    if info["count_init"]:
        want = (info["active"].double() / k - 1) / info["count_init"]
        err = ((gcv.sum(1, keepdim=True) - want).abs() * mask).max()
        assert float(err) <= 4 * np.spacing(np.float32(1.0 / info["count_init"])), float(err)
    if c[7]:
        assert bool(torch.isnan(total))
        for n in INPUTS:
            assert bool(torch.isfinite(got[n]).all()) and not got[n].any(), n


def test_determinism_retain_graph_and_partial_backward(dev, gold):
    from tcs_mi355 import train_losses as tl
    i, c = 4, [int(v) for v in gold["cases"][4]]
    case = case_inputs(c)
    runs = []
    for _ in range(2):
        L = Leaves(case, dev, c[4])
        total, _ = tl.training_objective(L.out, L.flow, L.valid, init_k=c[5], dense_gt=bool(c[6]), sync=False)
        a = L.grads(total, retain_graph=True)
        b = L.grads(total, retain_graph=True)
        for n in INPUTS:
            assert torch.equal(a[n], b[n]), n
            one = L.grads(total, (n,), retain_graph=True)[n]
            assert torch.equal(one, a[n]), n
        runs.append(a)
    for n in INPUTS:
        assert torch.equal(runs[0][n], runs[1][n]), n


def test_upstream_gradient_and_parts(dev, gold):
    """(3 * total).backward() is 3x; a device scalar (GradScaler's scale) works; the parts weighted by hand combine linearly."""
    from tcs_mi355 import train_losses as tl
    c = [int(v) for v in gold["cases"][0]]
    case = case_inputs(c)
    L = Leaves(case, dev, c[4])
    total, vec, parts = tl.training_objective(L.out, L.flow, L.valid, init_k=c[5], dense_gt=bool(c[6]), sync=False, return_parts=True)
    assert set(parts) == {"seq_loss", "init_loss", "norm_loss", "grad_loss"}
    assert torch.equal(torch.stack([parts[p] for p in ("seq_loss", "init_loss", "norm_loss", "grad_loss")]), vec[1:5].float())
    base = L.grads(total, retain_graph=True)
    tripled = L.grads(3 * total, retain_graph=True)
    scale = torch.full((), 1024.0, device=dev)
    scaled = L.grads(total * scale, retain_graph=True)
    for n in INPUTS:
        assert torch.equal(tripled[n], (3.0 * base[n].double()).float()) or float((tripled[n] - 3 * base[n]).abs().max()) <= float(
            np.spacing(np.float32(3 * base[n].abs().max().item()))), n
        assert torch.equal(scaled[n], 1024.0 * base[n]), n                      # a power of two: exact
    own = 2 * parts["seq_loss"] + 0.5 * parts["init_loss"] + parts["norm_loss"] + 3 * parts["grad_loss"]
    mine = L.grads(own, retain_graph=True)
    for part, wgt in (("seq_loss", 2.0), ("init_loss", 0.5), ("norm_loss", 1.0), ("grad_loss", 3.0)):
        names = PART_INPUTS[part.split("_")[0]]
        alone = L.grads(parts[part], names, retain_graph=True)
        for n in names:
            want = wgt * alone[n].double()
            assert float((mine[n].double() - want).abs().max()) <= float(np.spacing(np.float32(want.abs().max().item()))), (part, n)
    # sync=True: the metrics dict of losses, and a differentiable total
    total2, metrics = tl.training_objective(L.out, L.flow, L.valid, init_k=c[5], dense_gt=bool(c[6]))
    assert total2.grad_fn is not None and torch.equal(total2.detach(), total.detach()) and "epe" in metrics


def test_grad_off_is_the_value_only_objective(dev, gold):
    from tcs_mi355 import losses, train_losses as tl
    for i, c in _cases(gold):
        case = case_inputs(c)
        L = Leaves(case, dev, c[4])
        det = {key: ([[x.detach() for x in p] for p in val] if key != "disp_grad_q_predictions" else [x.detach() for x in val])
               if isinstance(val, list) else val.detach() for key, val in L.out.items()}
        want_t, want_v = losses.training_objective(det, L.flow, L.valid, init_k=c[5], dense_gt=bool(c[6]), sync=False)
        with torch.no_grad():
            t1, v1 = tl.training_objective(L.out, L.flow, L.valid, init_k=c[5], dense_gt=bool(c[6]), sync=False)
        t2, v2 = tl.training_objective(det, L.flow, L.valid, init_k=c[5], dense_gt=bool(c[6]), sync=False)
        t3, v3 = tl.training_objective(L.out, L.flow, L.valid, init_k=c[5], dense_gt=bool(c[6]), sync=False)
        for t, v in ((t1, v1), (t2, v2), (t3, v3)):
            assert torch.equal(t.detach().view(torch.int32), want_t.view(torch.int32)), i
            assert torch.equal(v.view(torch.int64), want_v.view(torch.int64)), i
        assert t1.grad_fn is None and t2.grad_fn is None and t3.grad_fn is not None


def test_double_backward_raises(dev, gold):
    from tcs_mi355 import train_losses as tl
    c = [int(v) for v in gold["cases"][0]]
    L = Leaves(case_inputs(c), dev, c[4])
    total, _ = tl.training_objective(L.out, L.flow, L.valid, sync=False)
    g, = torch.autograd.grad(total, [L.single["flow_mono"]], create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


def test_cost_volume_chain_reaches_the_feature_maps(dev, gold):
    """CorrBlock1D(want_cost_volume=True) -> get_cost_volume() -> init_loss -> backward, against the same chain in torch ops."""
    from tcs_mi355 import train_losses as tl
    from tcs_mi355.corr import CorrBlock1D
    c = [int(v) for v in gold["cases"][0]]
    case = case_inputs(c)
    flow, valid_raw = torch.from_numpy(case["flow"]), torch.from_numpy(case["valid"])
    v = targets(flow, valid_raw)[0]
    B, _, Hh, Ww = flow.shape
    gen = torch.Generator().manual_seed(11)
    f = [torch.randn(B, 256, Hh // 4, Ww // 4, generator=gen) for _ in range(2)]

    def chain(dtype):
        a, b = (x.clone().to(dtype).requires_grad_(True) for x in f)
        n1, n2 = torch.nn.functional.normalize(a, dim=1), torch.nn.functional.normalize(b, dim=1)
        vol = torch.einsum("aijk,aijh->ajkh", n1, n2).permute(0, 3, 1, 2)                  # [B, w2, h, w1]
        w = vol.shape[1]
        j = torch.arange(w)
        cv = vol * (j.view(1, w, 1, 1) <= j.view(1, 1, 1, w)).to(dtype)
        loss, _ = init_loss_torch(cv, flow, v, 3, 0.5)
        return torch.autograd.grad(loss, [a, b])
    g64, g32 = chain(torch.float64), chain(torch.float32)
    a, b = (x.clone().to(dev).requires_grad_(True) for x in f)
    blk = CorrBlock1D(a, b, want_cost_volume=True)
    loss, _ = tl.init_loss(blk.get_cost_volume(), flow.to(dev), v.to(dev), k=3, scale=0.25, threshold=0.5)
    loss.backward()
    for name, hip, x64, x32 in (("fmap1", a.grad, g64[0], g32[0]), ("fmap2", b.grad, g64[1], g32[1])):
        compare(f"chain {name}", hip, x64, x32, torch.zeros_like(x64, dtype=torch.bool))


def test_trainer_step(dev, gold):
    """A two-layer conv head makes the predictions from a seeded image; objective, backward, SGD step: the parameters after the step
    match the run that scores the same predictions with the objective in torch ops, to 1e-5 relative, and so do the gradients."""
    from tcs_mi355 import train_losses as tl
    c = [int(v) for v in gold["cases"][0]]
    case = case_inputs(c)
    iters, k, dense = c[4], c[5], bool(c[6])
    flow, valid = torch.from_numpy(case["flow"]).to(dev), torch.from_numpy(case["valid"]).to(dev)
    B, _, Hh, Ww = flow.shape
    h, w = Hh // 4, Ww // 4
    n_full, n_q = 2 * iters + 2, 2 * iters + 2 * iters + w               # up pairs + mono + init; q pairs + grad (2 ch) + cost volume

    def run(hip):
        torch.manual_seed(3)
        net = torch.nn.Sequential(torch.nn.Conv2d(3, 16, 3, padding=1), torch.nn.Tanh(), torch.nn.Conv2d(16, n_full + n_q, 3, padding=1)).to(dev)
        img = torch.rand(B, 3, Hh, Ww, generator=torch.Generator().manual_seed(4)).to(dev)
        y = net(img)
        full = y[:, :n_full] + flow                                     # near the ground truth, like a model's predictions
        quarter = torch.nn.functional.pixel_unshuffle(y[:, n_full:], 4).view(B, n_q, 16, h, w).mean(2)
        up = [[full[:, 2 * i:2 * i + 1], full[:, 2 * i + 1:2 * i + 2]] for i in range(iters)]
        fq = flow[:, :, ::4, ::4] / 4
        q = [[quarter[:, 2 * i:2 * i + 1] + fq, quarter[:, 2 * i + 1:2 * i + 2] + fq] for i in range(iters)]
        grad = [quarter[:, 2 * iters + 2 * i:2 * iters + 2 * i + 2] for i in range(iters)]
        out = {"flow_predictions": up, "flow_q_predictions": q, "disp_grad_q_predictions": grad, "flow_mono": full[:, 2 * iters:2 * iters + 1],
               "flow_init": full[:, 2 * iters + 1:2 * iters + 2], "cost_volume": quarter[:, 4 * iters:]}
        opt = torch.optim.SGD(net.parameters(), lr=0.05)
        if hip:
            total, _ = tl.training_objective(out, flow, valid, init_k=k, dense_gt=dense, sync=False)
        else:                                                           # the same objective in torch ops, on the CPU in float32
            Lc = {"up": torch.stack([torch.stack(p) for p in up]).cpu(), "q": torch.stack([torch.stack(p) for p in q]).cpu(),
                  "grad": torch.stack(grad).cpu(), "flow_mono": out["flow_mono"].cpu(), "flow_init": out["flow_init"].cpu(),
                  "cost_volume": out["cost_volume"].cpu()}
            total = objective_torch(Lc, flow.cpu(), valid.cpu(), iters, k, dense)[0]["total"]
        total.backward()
        opt.step()
        return float(total.detach()), [p.detach().cpu().double() for p in net.parameters()], [p.grad.detach().cpu().double() for p in net.parameters()]
    t_hip, p_hip, g_hip = run(True)
    t_ref, p_ref, g_ref = run(False)
    assert abs(t_hip - t_ref) <= 1e-5 * abs(t_ref), (t_hip, t_ref)
    for a, b, gh, gr in zip(p_hip, p_ref, g_hip, g_ref):
        assert float(gr.abs().max()) > 0
        rel = float((a - b).norm() / b.norm())
        # the gradients themselves, the stronger check: both runs share the convolutions' backward, and what enters it differs by the
        # objective's fp32 rounding only (a few 1e-7 of each tensor's largest gradient, test_training_objective_gradients), so 1e-5
        # of the gradient's norm leaves more than a decade of margin (each part's own gradient is checked per tensor above)
        rel_g = float((gh - gr).norm() / gr.norm())
        print(f"trainer step: parameter {tuple(a.shape)} relative difference {rel:.3e}, of its gradient {rel_g:.3e}")
        assert rel <= 1e-5, rel
        assert rel_g <= 1e-5, rel_g
