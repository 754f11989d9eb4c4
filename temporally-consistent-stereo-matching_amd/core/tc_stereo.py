"""Drop-in for the reference's core/tc_stereo.py: `TCStereo` with the hot path on MI355X.

Same constructor (an argparse-style Namespace), same sub-module names (reference checkpoints load
with strict=True), same `forward(image1, image2, iters, params, test_mode, frame_id)` signature and
the same test-mode output dict, so evaluate_stereo.py's loop (evaluate_stereo.py:170-197) runs
unchanged.  One optional addition: `prefetch(next_image1, next_image2)` for video loops (the next frame's
image-only stage is enqueued ahead of time).  What differs is underneath: correlation build/lookup, the temporal warp, the GRU update
step, both U-Nets, every stencil and the feature extractor's convolutions are hand-written HIP kernels
for gfx950 (libtcs_mi355.so); PyTorch-ROCm owns tensors, streams and graph capture.

No autograd: `test_mode=False` returns the reference's training-output dict (every iteration's predictions, the cost volume,
flow_mono / flow_init) under torch.no_grad() / inference_mode() or with frozen parameters, and raises NotImplementedError when
gradients would be expected.  There is no CPU path: tensors must live on a HIP device and the library must be built.
"""
import contextlib
import os

import torch
import torch.nn as nn

from core.corr import CorrBlock1D
from core.extractor import BasicEncoder, MultiBasicEncoder, ResidualBlock, hip_head
from core.update import (IN_SUM_SLOTS, BasicMultiUpdateBlock, DispGradPredictor, DispRefine, DisparityCompletor, HiddenstateUpdater,
                         Lightfuse, hip_conv)
from core.utils.utils import coords_grid
from tcs_mi355 import ops, s16


class autocast(contextlib.AbstractContextManager):
    """evaluate_stereo.py imports `autocast` from here (evaluate_stereo.py:14).  The HIP path keeps fp32 tensors and fp32-grade
    contractions (fp16 hi/lo split operands with fp32 accumulation, or fp32 MFMA — DESIGN.md section 5) whatever `enabled` says, so
    this is a no-op context."""

    def __init__(self, enabled=False, **_):
        self.enabled = enabled

    def __exit__(self, *exc):
        return False


# Arithmetic of the fp16-split convolutions per model instance (`args.hip_precision`, DESIGN.md section 5 / INTEGRATION.md):
#   "fp32" (default): fp16 hi/lo split operands, three MFMA products each, fp32 accumulation — fp32-grade results;
#   "fp16": the hi halves only, sum f16(x) * f16(w) with fp32 accumulation, one product (tcs_conv*_desc.products = 1).
# Storage, epilogues, every non-convolution kernel, the fp32 kernels (correlation, the gradient-candidate stem, the 7x7 stems) and the
# two small split contractions (fused HiddenstateUpdater, tap partials) are the same in both.  `mixed_precision` / `autocast` do not
# select it.
HIP_PRECISIONS = {"fp32": 0, "fp16": 1}


def sequence_starts(value, batch: int, device=None) -> torch.Tensor:
    """`params["new_sequence"]` validated and normalised: a bool / uint8 tensor of shape [batch] (host or device) or a Python sequence
    of `batch` bools -> a uint8 [batch] tensor on `device` (1 = the element begins a sequence).  A device tensor is converted on the
    device and never read on the host.  Raises ValueError for a wrong length, a wrong dtype or a mask that is not 1-D."""
    if torch.is_tensor(value):
        if value.ndim != 1:
            raise ValueError(f"new_sequence must be 1-D [{batch}], got shape {tuple(value.shape)}")
        if value.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"new_sequence must be a bool or uint8 tensor, got {value.dtype}")
        if int(value.shape[0]) != batch:
            raise ValueError(f"new_sequence has {int(value.shape[0])} entries for batch {batch}")
        t = value
    else:
        if isinstance(value, (str, bytes)) or not hasattr(value, "__len__"):
            raise ValueError(f"new_sequence must be a tensor or a sequence of {batch} bools, got {type(value).__name__}")
        vals = list(value)
        if len(vals) != batch:
            raise ValueError(f"new_sequence has {len(vals)} entries for batch {batch}")
        if not all(isinstance(v, bool) or type(v).__name__ in ("bool", "bool_") for v in vals):      # (numpy bools too)
            raise ValueError("new_sequence must hold bools (a nested or non-bool sequence is not a [B] mask)")
        t = torch.tensor([bool(v) for v in vals], dtype=torch.uint8)
    if device is not None and t.device != torch.device(device):
        t = t.to(device)
    return t.to(torch.uint8).contiguous()


class TCStereo(nn.Module):
    def __init__(self, args):
        super().__init__()
        precision = getattr(args, "hip_precision", "fp32")
        if precision not in HIP_PRECISIONS:
            raise ValueError(f"hip_precision must be one of {sorted(HIP_PRECISIONS)}, got {precision!r}")
        self._hip_precision = precision
        deterministic = getattr(args, "hip_deterministic", False)
        if not isinstance(deterministic, bool):
            raise ValueError(f"hip_deterministic must be a bool, got {deterministic!r}")
        self._hip_deterministic = deterministic
        self.args = args
        self.scale_rate = 1 / (2 ** args.n_downsample)
        hd = list(args.hidden_dims)
        n = args.n_gru_layers
        self.cnet = MultiBasicEncoder(output_dim=[hd, hd], norm_fn=args.context_norm, downsample=args.n_downsample)
        self.update_block = BasicMultiUpdateBlock(args, hidden_dims=hd)
        self.context_zqr_convs = nn.ModuleList([nn.Conv2d(hd[i], hd[i] * 3, 3, padding=1) for i in range(n)])
        if args.shared_backbone:
            self.conv2 = nn.Sequential(ResidualBlock(128, 128, "instance", stride=1), nn.Conv2d(128, 256, 3, padding=1))
        else:
            self.fnet = BasicEncoder(output_dim=256, norm_fn="instance", downsample=args.n_downsample)
        self.previous_current_hideen_fuse = nn.ModuleList([Lightfuse(hd[i], hd[i]) for i in range(n)])   # (sic)
        self.disp_completor = DisparityCompletor()
        self.disp_grad_refine = DispGradPredictor(args)
        self.disp_refine = DispRefine(args)
        self.context_zqr_convs_grad = nn.ModuleList([nn.Conv2d(hd[i], 64, 3, padding=1) for i in range(n)])
        self.hiddenstate_update = HiddenstateUpdater(hd[0])
        # one pool of pre-split ("S16") activation buffers for the whole model: allocated (zero-filled) on first use,
        # reused every iteration and frame (tcs_mi355/s16.py)
        pool = s16.S16Pool(products=HIP_PRECISIONS[precision])
        for m in self.modules():
            m._s16pool = pool
        # layers that stay fp16-split in both modes: the fused HiddenstateUpdater and the 3x3 convolutions to 1-2 channels that run folded
        # into their producer as tap partials (core/update.py: products_of)
        for m in self.hiddenstate_update.modules():
            m._tcs_x3 = True
        self.update_block.flow_head.conv2._tcs_x3 = True
        self.disp_grad_refine.residual_head[2]._tcs_x3 = True

    @property
    def hip_precision(self) -> str:
        """"fp32" or "fp16": the arithmetic of this model's fp16-split convolutions, fixed at construction (args.hip_precision)."""
        return self._hip_precision

    @property
    def hip_deterministic(self) -> bool:
        """True: the temporal warp's splat sums in a fixed order (ops.warp_forward(ordered=True)), so that every frame of a sequence is
        bit-reproducible from run to run; fixed at construction (args.hip_deterministic, default False: the float-atomic splat)."""
        return self._hip_deterministic

    def freeze_bn(self):
        for m in self.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.eval()

    def _coords0(self, img):
        """The x-coordinate grid at feature resolution, built once per shape (a constant of the frame)."""
        key = (int(img.shape[0]), int(img.shape[2]), int(img.shape[3]), str(img.device))
        cache = self.__dict__.setdefault("_coords0_cache", {})
        if key not in cache:
            cache[key] = coords_grid(key[0], key[1], key[2], device=img.device)[:, :1].contiguous()
        return cache[key]

    def initialize_flow(self, img):
        """coords0, coords1: the x-coordinate grid at feature resolution, [N,1,H,W] each (tc_stereo.py:66-73)."""
        n, _, h, w = img.shape
        g = coords_grid(n, h, w, device=img.device)[:, :1].contiguous()
        return g, g.clone()

    def upsample_flow(self, flow, mask, scale=True):
        """Convex x4 upsampling (tc_stereo.py:75-88).  Returns the upsampled flow (not clipped)."""
        if not scale or self.args.n_downsample != 2:
            raise NotImplementedError("HIP convex upsampling covers factor 4 with scaling")
        up, _ = ops.convex_upsample((-flow).float().contiguous(), mask.float().contiguous(), clip=False)   # kernel takes disparity
        return up

    def fuse_previous_current_hidden_state(self, net_list, warp_net_list):
        return [fuse(n, w) for n, w, fuse in zip(net_list, warp_net_list, self.previous_current_hideen_fuse)]

    def _weights_epoch(self):
        """Changes whenever a parameter tensor is replaced or written in place (load_state_dict, .copy_, optimiser step)."""
        return hash(tuple((p.data_ptr(), p._version) for p in self.parameters()))

    # -----------------------------------------------------------------------------------------
    def _features(self, image1, image2):
        a = self.args
        if a.shared_backbone:
            *cnet_list, trunk = self.cnet(torch.cat((image1, image2), 0), dual_inp=True, num_layers=a.n_gru_layers)
            fm = hip_head(self.conv2, trunk)                     # trunk: fp32 tensor, or an S16 tensor from the all-HIP context network
            fmap1, fmap2 = fm.split(fm.shape[0] // 2, 0)
        else:
            cnet_list = self.cnet(image1, num_layers=a.n_gru_layers)
            fmap1, fmap2 = self.fnet([image1, image2])
        return list(cnet_list), fmap1.float().contiguous(), fmap2.float().contiguous()

    def _pipeline(self):
        if getattr(self, "_graphs", None) is None:
            from tcs_mi355.graph import FrameGraphs
            self._graphs = FrameGraphs(self._extract_stage, self._refine_head, self._refine_loop, epoch_fn=self._weights_epoch,
                                       strict=os.environ.get("TCS_MI355_GRAPH_STRICT", "0") == "1")
        return self._graphs

    def _graph_mode(self):
        if getattr(self, "use_hip_graph", None) is None:
            self.use_hip_graph = os.environ.get("TCS_MI355_GRAPH", "1") != "0"
        return bool(self.use_hip_graph)

    @torch.no_grad()
    def prefetch(self, image1, image2, first=False, inputs_ready=False):
        """Optional, for callers that know the next frame (a video loop): enqueue the part of a frame that depends on nothing but its
        two images — feature / context networks, correlation pyramid, context convolutions (tc_stereo.py:101-116,147-149) — right
        behind the frame in flight on the caller's stream, so that its host-side launch work is done while the GPU is still busy with
        that frame.  The next `forward` with the SAME image tensors
        (same objects, unmodified) picks the result up; any other call simply extracts again.  `first`: that frame will be called with
        params=None (start of a sequence: the arg-max prior is then built with the correlation volume) or with
        params["new_sequence"] present (a mixed batch, which always takes the arg-max).  Call it right AFTER the
        `forward` it follows.  `inputs_ready` is accepted for existing callers and ignored.  Results are identical with and without
        the call."""
        if not image1.is_cuda:
            raise RuntimeError("TCStereo.prefetch needs HIP device tensors; there is no CPU fallback")
        self._pipeline().prefetch(image1, image2, first=bool(first), use_graph=self._graph_mode())

    def forward(self, image1, image2, iters=12, params=None, test_mode=False, frame_id=0):
        """Disparity of a stereo pair, optionally conditioned on the previous frame (`params`):
        K [b,3,3], T / previous_T [b,4,4] world->camera, baseline [b], last_disp (= previous 'flow_q'),
        last_net_list, fmap1.  Returns {'flow' [b,1,H,W] (negative disparity, clipped at 0),
        'flow_q' [b,1,H/4,W/4], 'net_list', 'fmap1'} (tc_stereo.py:96-244).

        Mixed batches (independent sequences on the batch dimension that start at different frames): `params["new_sequence"]`, a
        bool / uint8 [b] tensor (host or device) or a sequence of b bools.  With the key present (even all False) the frame takes the
        mixed path: an element marked True is computed as a first frame (arg-max prior, zero warped hidden states) and its temporal
        entries (previous_T, last_disp, last_net_list, fmap1; they must have the batch's shapes) are never read, so they may hold
        anything; an element marked False gets what a temporal call on the sub-batch of the temporal elements gives (the warp's
        metric mean covers their pixels only).  The mask is never read on the host.  Absent or None: exactly the temporal path.

        A frame is two fixed launch sequences with no host round trip — the image-only stage (`_extract_stage`) and the
        state-dependent stage (`_refine_stage`) — so by default each is captured once per (shape, iters, branch) into a HIP
        graph and replayed (tcs_mi355.graph); set TCS_MI355_GRAPH=0 or `model.use_hip_graph = False` for eager launches.

        `test_mode=False` returns the reference's training-output dict (tc_stereo.py:229-243) without an autograd graph:
        'flow_predictions' (`iters` pairs [flows_up, flow_refine_up], the unclipped convex x4 upsamplings of -disp_q and
        -refined_disp, [b,1,H,W] each), 'flow_q_predictions' (`iters` pairs [-disp_q, -refined_disp], [b,1,H/4,W/4]),
        'disp_grad_q_predictions' (`iters` refined gradients [b,2,H/4,W/4]), 'flow_mono' / 'flow_init' ([b,1,H,W]), 'cost_volume'
        ([b,W/4,H/4,W/4], masked) and the same 'flow_q', 'net_list', 'fmap1' as test mode.  The per-iteration entries are views into
        one stacked tensor per key (e.g. flow_predictions[k][1] is a view of a [iters,2,b,1,H,W] tensor); every call returns fresh
        storage that no later call overwrites.  It runs under torch.no_grad() / torch.inference_mode() or when no parameter
        requires grad; otherwise it raises NotImplementedError.  Each iteration's upsampling mask head runs off the critical chain
        (DESIGN.md section 12)."""
        if not test_mode and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError("TCStereo on MI355X builds no autograd graph: call test_mode=False under torch.no_grad() (or "
                                      "torch.inference_mode(), or with every parameter frozen), or use test_mode=True")
        with torch.no_grad():
            return self._forward(image1, image2, iters, params, bool(test_mode))

    def _forward(self, image1, image2, iters, params, test_mode):
        if iters < 1:
            raise ValueError("iters must be >= 1")
        if not image1.is_cuda:
            raise RuntimeError("TCStereo.forward needs HIP device tensors; there is no CPU fallback")
        temporal = None
        if params is not None:
            temporal = (params["K"], params["T"], params["previous_T"], params["baseline"], params["last_disp"],
                        list(params["last_net_list"]), params["fmap1"])
            if params.get("new_sequence") is not None:          # mixed batch: the mask is the 8th entry
                temporal = temporal + (sequence_starts(params["new_sequence"], int(image1.shape[0]), image1.device),)
        if test_mode:
            return self._pipeline()(image1, image2, iters, temporal, use_graph=self._graph_mode())
        out = self._pipeline()(image1, image2, iters, temporal, use_graph=self._graph_mode(), outputs=True)
        return self._training_output(out, iters)

    @staticmethod
    def _training_output(out, iters):
        """The loop's stacked outputs -> the reference's training_output dict (per-iteration entries are views)."""
        up, q, grad = out["up"], out["q"], out["grad"]
        return {"flow_mono": out["flow_mono"], "flow_init": out["flow_init"],
                "flow_predictions": [[up[k, 0], up[k, 1]] for k in range(iters)],
                "flow_q_predictions": [[q[k, 0], q[k, 1]] for k in range(iters)],
                "disp_grad_q_predictions": [grad[k] for k in range(iters)],
                "cost_volume": out["cost_volume"],
                "flow_q": out["flow_q"], "net_list": out["net_list"], "fmap1": out["fmap1"]}

    def _frame(self, image1, image2, iters, temporal, outputs=False):
        """One frame as a pure launch sequence on the current stream (both stages back to back)."""
        feats = self._extract_stage(image1, image2, temporal is None or len(temporal) == 8, outputs)
        return self._refine_loop(feats, self._refine_head(feats, temporal), iters, outputs)

    def _extract_stage(self, image1, image2, first, cost_volume=False):
        """Everything of a frame that depends only on its two images (tensors in, tensors out; capturable): matching features,
        correlation pyramid (+ the arg-max prior on a first frame), per-scale context terms (tc_stereo.py:101-116,147-149).
        `cost_volume`: the build also writes the masked cost volume (test_mode=False's 'cost_volume', corr.py:24-31)."""
        a = self.args

        def correlate(fmap1, fmap2):
            corr_fn = CorrBlock1D(fmap1, fmap2, radius=a.corr_radius, num_levels=a.corr_levels, thres=a.init_thres, want_argmax=first,
                                  want_cost_volume=cost_volume)
            return corr_fn, (corr_fn.argmax_disp() if first else None)

        def context(cnet_list, relu_done=False):
            """Per-scale context terms of the GRUs and of the gradient predictor (tc_stereo.py:151-156): once per frame.  cz | cr | cq
            stay the three thirds of the context convolution's output (channel-slice views; the GRU epilogues index them in place)."""
            inp = [x[1] if relu_done else torch.relu(x[1]) for x in cnet_list]
            grads = [hip_conv(conv, [i]) for i, conv in zip(inp, self.context_zqr_convs_grad)]
            zqr = [list(hip_conv(conv, [i]).chunk(3, 1)) for i, conv in zip(inp, self.context_zqr_convs)]
            return zqr, grads, [x[0] for x in cnet_list]

        if a.shared_backbone and self.cnet.can16(image1):
            # the matching side (feature head -> correlation build) and the context side (per-scale heads -> context convolutions)
            # both start from the shared trunk: parallel graph branches.  The 7x7 stem reads the raw left | right images: the
            # normalisation to [-1, 1] and the batch concatenation (tc_stereo.py:101-107) happen in its input staging.
            from tcs_mi355.streams import fork_join
            trunk = self.cnet.trunk16(image1, right=image2, raw_images=True)

            def matching_side():
                fm = hip_head(self.conv2, trunk)
                f1, f2 = (t.float().contiguous() for t in fm.split(fm.shape[0] // 2, 0))
                return f1, f2, correlate(f1, f2)

            (fmap1, fmap2, (corr_fn, prior)), (inp_list, grad_list, net_list) = fork_join(
                [matching_side, lambda: context(self.cnet.heads16(trunk, True, a.n_gru_layers, relu_context=True), relu_done=True)])
        else:
            image1 = (2 * (image1 / 255.0) - 1.0).contiguous()
            image2 = (2 * (image2 / 255.0) - 1.0).contiguous()
            cnet_list, fmap1, fmap2 = self._features(image1, image2)
            corr_fn, prior = correlate(fmap1, fmap2)
            inp_list, grad_list, net_list = context(cnet_list)
        return {"fmap1": fmap1, "corr_fn": corr_fn, "prior": prior, "inp_list": inp_list, "grad_list": grad_list, "net_list": net_list}

    def _refine_head(self, feats, temporal):
        """The state-dependent head of a frame (tensors in, tensors out; capturable): prior from the arg-max or from the pose warp of the
        previous frame, disparity completion, hidden-state warp and fusion (tc_stereo.py:119-172) -> what the loop starts from."""
        first = temporal is None
        start = temporal[7] if temporal is not None and len(temporal) == 8 else None     # mixed batch: uint8 [B] sequence starts
        fmap1, corr_fn = feats["fmap1"], feats["corr_fn"]
        net_list = feats["net_list"]
        if first:
            last_net_list = None
            sparse_disp, cost, sparse_mask = feats["prior"] if feats["prior"] is not None else corr_fn.argmax_disp()
        else:
            K, T, previous_T, baseline, last_disp, last_net_list, last_fmap1 = temporal[:7]
            # K_scale, its inverse, T @ inv(previous_T), previous_T @ inv(T): one tiny kernel, no host sync (identity poses for the
            # start elements of a mixed batch)
            K_scale, K_scale_inv, relative_T, back_T = ops.pose_prepare(K, T, previous_T, self.scale_rate, start=start)
            # a mixed batch's start elements take the arg-max prior, selected inside the warp's finish kernel
            prior = None if start is None else (feats["prior"] if feats["prior"] is not None else corr_fn.argmax_disp())
            # warp + normalise + cosine cost in one launch sequence; the warped feature map is never materialised
            sparse_disp, _, sparse_mask, cost = ops.warp_forward(
                (-last_disp).float().contiguous(), last_fmap1.float().contiguous(), relative_T, K_scale,
                K_scale_inv, baseline, cur_fmap=fmap1, want_fmap=False, ordered=self._hip_deterministic, start=start, prior=prior)

        pool = self._s16pool
        disp_init, disp_mono, _, net_list = self.disp_completor.run16(pool, sparse_disp, cost, sparse_mask,
                                                                      [c.float().contiguous() for c in net_list], tanh_nets=True)
        disp_init = disp_init.float().contiguous()

        if last_net_list is None:
            warped = None
        else:
            grid = ops.backward_grid(disp_init, back_T, K_scale, K_scale_inv, baseline)
            warped = []
            for i, net in enumerate(last_net_list):
                warped.append(ops.bilinear_sample(net.float().contiguous(), grid, start=start))   # (+0.0 for start elements)
                if i + 1 < len(last_net_list):
                    grid = ops.grid_halve(grid)

        # previous / current hidden-state fusion (tc_stereo.py:167-168; tanh applied by the completor's last convolutions): the three
        # Lightfuse cells on S16 tensors, updating the completor's hidden states in place; a first frame fuses with zeros
        for i, (h, fuse) in enumerate(zip(net_list, self.previous_current_hideen_fuse)):
            if warped is None:
                x = pool.get(("frame", "zero", i), h.B, h.C, h.H, h.W, h.device)          # never written: stays zero
            else:
                x = s16.to_s16(warped[i], out=pool.get(("frame", "warped", i), h.B, h.C, h.H, h.W, h.device))
            fuse.step16(pool, h, [x])

        coords0 = self._coords0(fmap1)
        coords1 = (coords0 - disp_init).contiguous()
        trace = getattr(self, "_trace", None)          # debugging hook (eager mode only): intermediate tensors
        if trace is not None:
            trace.update(sparse_disp=sparse_disp, cost=cost, sparse_mask=sparse_mask, disp_init=disp_init,
                         net0=[t.float().clone() for t in net_list], iters=[])
        # (disp_init / disp_mono: read only by the outputs mode of the loop, for flow_init / flow_mono)
        return {"coords1": coords1, "net_list": net_list, "disp_init": disp_init, "disp_mono": disp_mono}

    def _refine_loop(self, feats, start, iters, outputs=False):
        """The refinement loop and the upsampling (tc_stereo.py:175-229) from the head's disparity / hidden states (capturable).
        `outputs` (test_mode=False): also every iteration's predictions, stacked, plus flow_mono / flow_init / cost_volume."""
        a = self.args
        fmap1, corr_fn = feats["fmap1"], feats["corr_fn"]
        inp_list, grad_list = feats["inp_list"], feats["grad_list"]
        # (hidden states: the S16 tensors the head's completor / Lightfuse cells left, updated in place by the loop)
        coords1, nets = start["coords1"], start["net_list"]
        coords0 = self._coords0(fmap1)
        trace = getattr(self, "_trace", None)

        # ---- refinement loop on pre-split activations (tcs_mi355/s16.py): hidden states, context features and the motion
        # feature buffer live in S16 pool buffers; 1-2 channel geometry (coords, disparity, gradients) stays fp32 ----
        pool = self._s16pool
        n3 = a.n_gru_layers == 3
        grads16 = [s16.to_s16(t.float().contiguous(), out=pool.get(("frame", "ctxg", i), t.shape[0], t.shape[1], t.shape[2], t.shape[3], t.device))
                   for i, t in enumerate(grad_list)]
        dg_pre = self.disp_grad_refine.prepare(pool, grads16)      # the context share of three convolutions: once per frame
        self.disp_grad_refine.begin_frame(pool, coords1.shape[0], coords1.device)
        refined = up_mask = None
        # coords1 - coords0, the motion encoder's flow input (tc_stereo.py:180): once here, afterwards the blend kernel writes
        # it for the next iteration — as a tensor for the 7x7 stem and into channel 127 of the motion feature buffer
        flows_x = (coords1 - coords0).contiguous()
        motion = pool.get(("frame", "motion"), coords1.shape[0], 128, coords1.shape[2], coords1.shape[3], coords1.device)
        s16.set_channel(flows_x, motion, 127)
        ub = self.update_block
        ub.begin_frame()
        from tcs_mi355.streams import fork_join, join, mark, spawn
        hu_delta = None              # the hidden-state update of iteration i-1 runs at the head of iteration i's coarse chain
        early32 = None               # gru32 of iteration i + the early share of gru16, launched during iteration i-1
        plain = not a.slow_fast_gru and n3
        side = _OutputsSide(self, pool, coords1, iters, start) if outputs else None
        # Schedule of one iteration.  The critical chain — blend(i-1) -> hidden-state update -> pool -> gru16's late
        # share -> interp -> gru08 -> flow head -> gradient predictor -> refinement -> blend(i) — is the FIRST branch of every fork, so
        # that it stays in one launch list of the captured graph (tcs_mi355/streams.py: capture order at a fork); what has slack hangs off it as side
        # branches: [corr lookup -> motion encoder] (needs only coords1 / the flow of the previous blend, due at gru08), and [gru32 of
        # the NEXT iteration -> the share of gru16 that reads only net16 / interp(net32)] (needs net16, due ~500 us later), forked at the
        # iteration's join but enqueued after gru08 / the flow head, so that gru08 and not this branch continues the launch list.
        # (Measured alternatives, profiles/r04_ab_logs.txt: the encoder chain as the first branch +1.3 ms; the early gru32 branch forked behind the
        # flow head's stencil instead of at the join +0.27 ms — on this stack the branch starts ~430 us into the iteration whichever node it hangs off.)
        for itr in range(iters):
            def enc_branch():
                corr = corr_fn(coords1)
                return corr, ub.encoder.run(pool, flows_x, corr, motion)

            def coarse_branch():
                if hu_delta is not None:
                    self.hiddenstate_update.run(pool, nets[0], hu_delta)
                if up32_now is not None:                 # gru32 ran ahead together with the early share of gru16
                    return ub.gru16_late(pool, nets, up32_now[1])
                if n3 and a.slow_fast_gru:
                    ub.run_coarse(pool, nets, inp_list, iter16=False, iter32=True, want_up16=False)
                if a.n_gru_layers >= 2 and a.slow_fast_gru:
                    ub.run_coarse(pool, nets, inp_list, iter16=True, iter32=n3, want_up16=False)
                return ub.run_coarse(pool, nets, inp_list, iter16=a.n_gru_layers >= 2, iter32=n3, up32=up32_now)

            up32_now = join(early32)                     # (None on the first iteration: gru32 then runs inside the coarse branch)
            early32 = None
            up16, (corr, m) = fork_join([coarse_branch, enc_branch])
            if side is not None:
                side.launch()                            # the previous iteration's mask head + pair upsampling (behind the blend)
            run_ahead = plain and trace is None and itr + 1 < iters
            # net16 is final for this iteration: gru32 of the NEXT iteration + gru16's early share (update.py) may start from here
            def ahead():
                up32 = ub.run_gru32(pool, nets, inp_list)
                return up32, ub.gru16_early(pool, nets, inp_list, up32)
            at_join = mark() if run_ahead else None                # forked HERE, enqueued behind gru08 / the flow head (never the join's first child)
            sums = getattr(self, "_checksums", None)       # debugging hook (tools/determinism_check.py): device-side sums, no sync
            lazy = trace is None and sums is None           # the hooks want the flow head's / residual head's outputs as tensors
            delta_flow = ub.run_fine(pool, nets, inp_list, m, up16, lazy=lazy)
            if at_join is not None:
                early32 = spawn(ahead, after=at_join)
            # disp_q = x - (coords1 + delta), 5 * disp2disp_gradient_xy (update.py:199) and the gradient candidates in one
            # launch (with the flow head's last convolution finished from its tap partials); coords1 is replaced by the blend
            # kernel's output below
            if isinstance(delta_flow, s16.Taps):
                disp_q, g5, cands = s16.flow_taps_step_grads(coords1, delta_flow, scale=5.0)
            else:
                disp_q, g5, cands = ops.flow_step_grads(coords1, delta_flow, scale=5.0)
            disp_grad, context = self.disp_grad_refine.run(pool, g5, cands, dg_pre, lazy=lazy, slot=itr if itr < IN_SUM_SLOTS else None)
            last = itr == iters - 1
            # (not on the last iteration: no lookup follows)
            warm = corr_fn._pyr if (not last and a.corr_levels == 4) else None
            if side is None:
                refined, up_mask, fused = self.disp_refine.run(pool, disp_grad, disp_q, nets[0], context, want_mask=last, motion=motion,
                                                               warm_pyramid=warm, warm_radius=a.corr_radius)
            else:
                refined, up_mask, fused = self.disp_refine.run(pool, disp_grad, disp_q, nets[0], context, motion=motion,
                                                               warm_pyramid=warm, warm_radius=a.corr_radius, grad_out=side.grad[itr],
                                                               before_fuse=side.join)
                side.record(itr, disp_q, refined, fused["fused"])
            hu_delta = fused["delta_disp"]
            coords1, flows_x = fused["coords1"], fused["flow_x"]
            if sums is not None:
                sums.append({k: v.double().sum() for k, v in dict(
                    corr=corr, motion=m.data, net0=nets[0].data, net1=nets[1].data, net2=nets[2].data, delta_flow=delta_flow,
                    disp_grad=disp_grad, context=context.data, refined=refined, coords1=coords1).items()})
            if trace is not None:
                self.hiddenstate_update.run(pool, nets[0], hu_delta)       # debugging hook: states as of the end of the iteration
                hu_delta = None
                trace["iters"].append(dict(corr=corr, delta=delta_flow, disp_q=disp_q, refined=refined,
                                           net=[t.float() for t in nets]))
        if hu_delta is not None:
            self.hiddenstate_update.run(pool, nets[0], hu_delta)
        if side is not None:
            side.launch()
            up_mask = side.join()                        # the last iteration's mask
        net_list = [t.float() for t in nets]

        flow_up, flow_q = ops.convex_upsample(refined.contiguous(), up_mask)
        out = {"flow": flow_up, "flow_q": flow_q, "net_list": [x.detach() for x in net_list], "fmap1": fmap1.detach()}
        if side is not None:
            out.update(side.outputs(corr_fn))
        return out


class _OutputsSide:
    """The outputs mode of `TCStereo._refine_loop` (test_mode=False).  Every iteration's upsampling mask head
    (DispRefine.mask_head, 6.4 GMAC at 640x480) and the pair kernel that upsamples disp_q and refined_disp with it only feed outputs, so
    they run as one side list (`streams.spawn`) per iteration, forked at the iteration's blend and enqueued behind the next launch of
    the critical chain (the hidden-state update), so that the chain stays its first child (tcs_mi355/streams.py, capture order).

    Hazard: the mask head reads DispRefine's pooled `fused` buffer, which the next iteration's conv_fuse[2] overwrites.  Chosen: the
    side list is joined right before that write (DispRefine.run(before_fuse=)).  It has the whole next iteration up to conv_fuse
    (~0.9 of an iteration) to finish, so the join rarely waits, and one join also orders the side lists among themselves, so that
    one set of side buffers (the mask head's S16 hidden layer, the fp32 mask) serves every iteration.  Two `fused` buffers by parity
    would change the default path's buffers or add a copy, and would still need a join two iterations later."""

    def __init__(self, model, pool, coords1, iters, start):
        B, _, H, W = (int(v) for v in coords1.shape)
        dev = coords1.device
        self.model, self.pool = model, pool
        # the stacked outputs: [iters, (disp_q, refined), B, 1, ...] and the refined gradients [iters, B, 2, H, W]
        self.up = torch.empty(iters, 2, B, 1, 4 * H, 4 * W, dtype=torch.float32, device=dev)
        self.q = torch.empty(iters, 2, B, 1, H, W, dtype=torch.float32, device=dev)
        self.grad = torch.empty(iters, B, 2, H, W, dtype=torch.float32, device=dev)
        self.mask = pool.get32((id(model.disp_refine.mask[2]), "outputs"), (B, 144, H, W), dev)
        self.flow_mono = torch.empty(B, 1, 4 * H, 4 * W, dtype=torch.float32, device=dev)
        self.flow_init = torch.empty_like(self.flow_mono)
        self.disp_mono, self.disp_init = start["disp_mono"].float().contiguous(), start["disp_init"].float().contiguous()
        self.pending = None         # (fork event, itr, disp_q, refined, fused) recorded at a blend, not yet launched
        self.running = None         # the spawned side list not yet joined
        self.keep = []              # every tensor a side list reads stays referenced until the loop's last join (eager allocator)

    def record(self, itr, disp_q, refined, fused):
        from tcs_mi355.streams import mark
        self.pending = (mark(), itr, disp_q, refined, fused)
        self.keep += [disp_q, refined]

    def launch(self):
        if self.pending is None:
            return
        from tcs_mi355.streams import spawn
        at, itr, disp_q, refined, fused = self.pending
        self.pending = None

        def side():
            if itr == 0:            # flow_mono / flow_init (tc_stereo.py:233-234): the head's outputs, ready long since
                H4, W4 = self.flow_mono.shape[-2:]
                ops.resize_bilinear(self.disp_mono, H4, W4, out=self.flow_mono, scale=-4.0)
                ops.resize_bilinear(self.disp_init, H4, W4, out=self.flow_init, scale=-4.0)
            self.model.disp_refine.mask_head(self.pool, fused, out=self.mask)
            ops.convex_upsample_pair(disp_q, refined, self.mask, self.up[itr, 0], self.up[itr, 1], self.q[itr, 0], self.q[itr, 1])

        self.running = spawn(side, slot=1, after=at)

    def join(self):
        from tcs_mi355.streams import join
        if self.running is not None:
            join(self.running)
            self.running = None
        return self.mask

    def outputs(self, corr_fn):
        self.keep = []
        return {"up": self.up, "q": self.q, "grad": self.grad, "flow_mono": self.flow_mono, "flow_init": self.flow_init,
                "cost_volume": corr_fn.get_cost_volume()}
