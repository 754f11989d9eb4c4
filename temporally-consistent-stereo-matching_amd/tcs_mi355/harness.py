"""Evaluation harness around the hot path: the caller side of `TCStereo.forward`.

Counterpart of validate_tartanair / validate_temporal_things (evaluate_stereo.py:119-223,264-345):
pads each frame (and shifts K), threads the temporal state dict through the model, and accumulates
EPE / D1 / D3 with the reference's validity mask and mask-rate weighting.  No wandb, no datasets:
sequences come from `tcs_mi355.synth` (or from files, when present, via `tcs_mi355.formats`).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence as Seq

import numpy as np
import torch
import torch.nn.functional as F


class InputPadder:
    """Replicate-pad [.., H, W] tensors up to a multiple of `divis_by` and move the principal point
    of K by the left/top pad (core/utils/utils.py:7-48).  'sintel' mode splits the padding evenly,
    any other mode pads bottom only (and left/right evenly)."""

    def __init__(self, dims, mode: str = "sintel", divis_by: int = 8):
        self.ht, self.wd = int(dims[-2]), int(dims[-1])
        extra_h = -self.ht % divis_by
        extra_w = -self.wd % divis_by
        left = extra_w // 2
        if mode == "sintel":
            top = extra_h // 2
        else:
            top = 0
        self.left, self.right, self.top, self.bottom = left, extra_w - left, top, extra_h - top

    def _shift(self, K, sign):
        K = K.clone()
        K[..., 0, 2] += sign * self.left
        K[..., 1, 2] += sign * self.top
        return K

    def pad(self, *tensors, K=None):
        """Like the reference (core/utils/utils.py:19-28): the bare list of padded tensors when `K` is None
        (`image1, image2 = padder.pad(image1, image2)`, evaluate_stereo.py:239), `(list, shifted K)` otherwise."""
        for t in tensors:
            if t.ndim != 4:
                raise ValueError("InputPadder.pad expects [N,C,H,W] tensors")
        padded = [F.pad(t, [self.left, self.right, self.top, self.bottom], mode="replicate") for t in tensors]
        return padded if K is None else (padded, self._shift(K, +1))

    def unpad(self, x, K=None):
        if x.ndim != 4:
            raise ValueError("InputPadder.unpad expects a [N,C,H,W] tensor")
        h, w = x.shape[-2:]
        y = x[..., self.top:h - self.bottom, self.left:w - self.right]
        return y if K is None else (y, self._shift(K, -1))


@dataclass
class FrameStats:
    epe: float
    d1_weighted: float       # mean(epe>1 over valid) * mask_rate
    d3_weighted: float
    mask_rate: float


@dataclass
class SequenceStats:
    frames: List[FrameStats] = field(default_factory=list)
    domain_flags: int = 0        # tcs_s16_flags after the sequence: bit 0 = an activation was clamped at +-65504, bit 1 = NaN / Inf seen
    # run_sequence(per_iteration=True): per_iteration[f][k] = frame_metrics of scored frame f (aligned with `frames`) after iteration k+1
    per_iteration: List[List[FrameStats]] = field(default_factory=list)
    # run_sequence(objective=True): objective[f] = training_objective's metrics dict of frame f (every frame, scored or not)
    objective: List[Dict[str, float]] = field(default_factory=list)

    def iteration_epe(self) -> np.ndarray:
        """Mean EPE over the scored frames at every iteration count: [iters] (empty without per_iteration)."""
        rows = [[f.epe for f in fr] for fr in self.per_iteration]
        return np.array(rows, np.float64).mean(0) if rows else np.zeros(0, np.float64)

    def vector(self) -> np.ndarray:
        """[sum_epe, sum_d1w, sum_d3w, sum_rate, n_frames]: what one rank contributes to the gather."""
        if not self.frames:
            return np.zeros(5, np.float64)
        a = np.array([[f.epe, f.d1_weighted, f.d3_weighted, f.mask_rate, 1.0] for f in self.frames], np.float64)
        return a.sum(0)


def frame_metrics(disp_pr: torch.Tensor, disp_gt: torch.Tensor, max_disp: float = 192.0) -> Optional[FrameStats]:
    """evaluate_stereo.py:201-213: per-pixel |pr-gt|, valid = |gt| < 192, outlier rates at 1 and 3 px,
    weighted by the fraction of valid pixels.  Returns None when no pixel is valid (frame skipped)."""
    if disp_pr.shape != disp_gt.shape:
        raise ValueError(f"shape mismatch {tuple(disp_pr.shape)} vs {tuple(disp_gt.shape)}")
    err = (disp_pr - disp_gt).abs().flatten()
    valid = disp_gt.abs().flatten() < max_disp
    if not bool(valid.any()):
        return None
    rate = float(valid.float().mean())
    e = err[valid]
    return FrameStats(float(e.mean()), float((e > 1.0).float().mean()) * rate, float((e > 3.0).float().mean()) * rate, rate)


def reduce_stats(vectors: Seq[np.ndarray]) -> Dict[str, float]:
    """evaluate_stereo.py:214-220: epe = mean over frames; d1 = 100*mean(out*rate)/mean(rate)."""
    tot = np.sum(np.stack(vectors, 0), 0)
    n = max(tot[4], 1.0)
    rate = max(tot[3] / n, 1e-12)
    return {"epe": tot[0] / n, "d1": 100.0 * (tot[1] / n) / rate, "d3": 100.0 * (tot[2] / n) / rate, "frames": int(tot[4])}


@torch.no_grad()
def run_sequence(forward: Callable, seq, iters: int, device, temporal: bool = True, divis_by: int = 32,
                 collect: Optional[list] = None, per_iteration: bool = False, objective: bool = False) -> SequenceStats:
    """One video sequence through `forward(image1, image2, iters=, test_mode=True, params=)`.
    State is reset per sequence (evaluate_stereo.py:170-174) and carried frame to frame
    (evaluate_stereo.py:182-197).  `collect`, if given, receives each frame's unpadded prediction.

    `per_iteration=True`: every frame is called with test_mode=False under torch.no_grad() and `stats.per_iteration[f][k]` gets the
    metrics of clip(flow_predictions[k][1], max=0), k = 0 .. iters-1 (the frame's own metrics are those of the last entry, which
    equals test mode's 'flow').  The state carried forward (flow_q, net_list, fmap1) is the N-iteration one, as in test mode.  So
    entry k of a frame is what a (k+1)-iteration run of THAT frame gives, given the N-iteration history of the frames before it —
    not a sequence run with k+1 iterations throughout (from the second frame on the two differ).

    `objective=True` (needs iters >= 2): every frame is called with test_mode=False under torch.no_grad() and scored with
    tcs_mi355.losses.training_objective against its disp_gt (flow = -disp_gt, valid where |disp_gt| < 192; the padding is
    invalid); `stats.objective[f]` gets the metrics dict plus 'loss'."""
    stats = SequenceStats()
    K_raw = torch.as_tensor(seq.K, dtype=torch.float32, device=device)[None]
    baseline = torch.tensor([seq.baseline], dtype=torch.float32, device=device)
    params: dict = {}
    flow_q = fmap1 = prev_T = nets = None
    for fr in seq.frames:
        im1 = torch.as_tensor(fr.image1, device=device)[None]
        im2 = torch.as_tensor(fr.image2, device=device)[None]
        gt = torch.as_tensor(fr.disp_gt, device=device)[None]
        T = torch.as_tensor(fr.T, device=device)[None]
        padder = InputPadder(im1.shape, divis_by=divis_by)
        (im1, im2), K = padder.pad(im1, im2, K=K_raw)
        params.update(K=K, T=T, previous_T=prev_T, last_disp=flow_q, last_net_list=nets, fmap1=fmap1, baseline=baseline)
        call_params = params if (flow_q is not None and temporal) else None
        if per_iteration or objective:
            with torch.no_grad():
                out = forward(im1, im2, iters=iters, test_mode=False, params=call_params)
        if objective:
            from .losses import training_objective
            pads = [padder.left, padder.right, padder.top, padder.bottom]
            flow_gt = F.pad(-gt.float(), pads)                     # gt: [1,1,H,W]
            valid = F.pad((gt.abs() < 192.0).float(), pads)
            total, metrics = training_objective(out, flow_gt.contiguous(), valid.contiguous())
            stats.objective.append({"loss": float(total), **metrics})
        if per_iteration:
            curve = [frame_metrics(padder.unpad(-torch.clip(p[1], max=0)), gt) for p in out["flow_predictions"]]
            disp_pr = padder.unpad(-torch.clip(out["flow_predictions"][-1][1], max=0))
        elif objective:
            disp_pr = padder.unpad(-torch.clip(out["flow_predictions"][-1][1], max=0))
        else:
            out = forward(im1, im2, iters=iters, test_mode=True, params=call_params)
            disp_pr = padder.unpad(-out["flow"])
        flow_q, nets, fmap1, prev_T = out["flow_q"], out["net_list"], out["fmap1"], T
        if collect is not None:
            collect.append(disp_pr)
        fs = frame_metrics(disp_pr, gt)
        if fs is not None:
            stats.frames.append(fs)
            if per_iteration:
                stats.per_iteration.append(curve)
    if torch.device(device).type == "cuda":
        # the device-side replacement of the reference's per-iteration NaN asserts: one read per sequence
        from . import s16
        stats.domain_flags = s16.take_flags()
        if stats.domain_flags:
            import warnings
            warnings.warn(f"activations left the fp16-split domain during this sequence (flags {stats.domain_flags:#x}: "
                          f"bit 0 = clamped at 65504, bit 1 = NaN/Inf)")
    return stats


def _padded_shape(seq, divis_by: int):
    f = seq.frames[0]
    p = InputPadder(np.shape(f.image1), divis_by=divis_by)
    return (int(np.shape(f.image1)[0]), p.ht + p.top + p.bottom, p.wd + p.left + p.right)


@torch.no_grad()
def run_sequences(forward: Callable, seqs, iters: int, device, batch: int, temporal: bool = True, divis_by: int = 32,
                  collect: Optional[list] = None, prefetch: bool = False) -> List[SequenceStats]:
    """Continuous batching: the sequences `seqs` through `forward` over `batch` slots of one batch dimension, each slot running one
    sequence at a time.  A slot whose sequence has ended takes the next one, and that element is called with
    `params["new_sequence"][slot] = True` (TCStereo.forward's mixed batch: a first frame for it, a temporal frame for the others).
    The first call is `params=None`; a call in which no slot starts a sequence carries no `new_sequence` key (the temporal path).
    K, T and baseline are stacked per slot and the state is threaded per slot as `run_sequence` threads it.  The batch stays
    `batch` wide: a slot with nothing left to run holds a padding element (zero images, marked as a sequence start) whose outputs
    are discarded and never counted, so no new shape is captured.  Sequences are taken longest first (a shorter padded tail);
    the results do not depend on the input order.

    Returns one `SequenceStats` per sequence, in input order, with `run_sequence`'s per-frame metrics; `collect`, if given,
    receives one list per sequence (input order) of its unpadded predictions.  `domain_flags` is RUN-level: the device-side flags
    are read once, after the last call, and every sequence of the run reports that value.  `temporal=False` calls every frame with
    params=None.  Sequences whose padded shapes differ raise ValueError.  `prefetch=True` needs `forward` to be a TCStereo: each
    call is followed by `forward.prefetch` of the next call's images (`first=True` when any slot starts on that call)."""
    seqs = list(seqs)
    if batch < 1:
        raise ValueError("batch must be >= 1")
    if prefetch:
        from core.tc_stereo import TCStereo
        if not isinstance(forward, TCStereo):
            raise ValueError("run_sequences(prefetch=True) needs a TCStereo as `forward` (it calls forward.prefetch)")
    stats = [SequenceStats() for _ in seqs]
    preds: List[list] = [[] for _ in seqs]
    if seqs:
        shapes = {_padded_shape(q, divis_by) for q in seqs}
        if len(shapes) > 1:
            raise ValueError(f"run_sequences needs one padded shape for all sequences, got {sorted(shapes)}")
    queue = sorted(range(len(seqs)), key=lambda i: (-len(seqs[i].frames), i))     # longest first; ties in input order
    queue = [i for i in queue if seqs[i].frames]
    slot_seq: List[Optional[int]] = [None] * batch      # the sequence a slot runs, None = idle (padding)
    slot_pos = [0] * batch                              # its next frame
    pad_like = None                                     # (a real slot's inputs: shapes and a finite K / T for padding elements)

    def assign():
        """Fill idle slots from the queue; -> the per-slot sequence-start flags of the coming call."""
        starts = []
        for b in range(batch):
            if slot_seq[b] is not None and slot_pos[b] >= len(seqs[slot_seq[b]].frames):
                slot_seq[b] = None
            if slot_seq[b] is None and queue:
                slot_seq[b], slot_pos[b] = queue.pop(0), 0
            starts.append(slot_seq[b] is None or slot_pos[b] == 0)
        return starts

    def inputs():
        """The stacked inputs of the coming call: padded images, shifted K, T, baseline, and the padders / ground truth per slot."""
        nonlocal pad_like
        per = []
        for b in range(batch):
            i = slot_seq[b]
            if i is None:
                per.append(None)
                continue
            q = seqs[i]
            fr = q.frames[slot_pos[b]]
            im1 = torch.as_tensor(fr.image1, device=device)[None]
            im2 = torch.as_tensor(fr.image2, device=device)[None]
            padder = InputPadder(im1.shape, divis_by=divis_by)
            K_raw = torch.as_tensor(q.K, dtype=torch.float32, device=device)[None]
            (im1, im2), K = padder.pad(im1, im2, K=K_raw)
            T = torch.as_tensor(fr.T, device=device)[None]
            base = torch.tensor([q.baseline], dtype=torch.float32, device=device)
            per.append((im1, im2, K, T, base, padder, torch.as_tensor(fr.disp_gt, device=device)[None]))
            if pad_like is None:
                pad_like = per[-1]
        rows = [p if p is not None else (torch.zeros_like(pad_like[0]), torch.zeros_like(pad_like[1]), pad_like[2], pad_like[3],
                                         pad_like[4], None, None) for p in per]
        cat = lambda k: torch.cat([r[k] for r in rows], 0)
        return cat(0), cat(1), cat(2), cat(3), cat(4), rows

    starts = assign()
    nxt = inputs() if any(s is not None for s in slot_seq) else None
    first_call = True
    prev_T = out = None
    while nxt is not None:
        im1, im2, K, T, base, rows = nxt
        if first_call or not temporal:
            params = None
        else:
            params = {"K": K, "T": T, "previous_T": prev_T, "baseline": base, "last_disp": out["flow_q"],
                      "last_net_list": out["net_list"], "fmap1": out["fmap1"]}
            if any(starts):
                params["new_sequence"] = torch.tensor(starts, dtype=torch.bool, device=device)
        running = list(slot_seq)
        out = forward(im1, im2, iters=iters, test_mode=True, params=params)
        first_call = False
        # previous_T of a start element is never read: its current T keeps the stacked tensor finite
        prev_T = T
        for b in range(batch):
            slot_pos[b] += int(running[b] is not None)
        starts = assign()
        nxt = inputs() if any(s is not None for s in slot_seq) else None
        if prefetch and nxt is not None:
            forward.prefetch(nxt[0], nxt[1], first=(not temporal) or any(starts))
        for b, i in enumerate(running):
            if i is None:
                continue                                          # padding: discarded
            padder, gt = rows[b][5], rows[b][6]
            disp_pr = padder.unpad(-out["flow"][b:b + 1])
            preds[i].append(disp_pr)
            fs = frame_metrics(disp_pr, gt)
            if fs is not None:
                stats[i].frames.append(fs)
    if torch.device(device).type == "cuda":
        from . import s16
        flags = s16.take_flags()
        for st in stats:
            st.domain_flags = flags
        if flags:
            import warnings
            warnings.warn(f"activations left the fp16-split domain during this run (flags {flags:#x}: "
                          f"bit 0 = clamped at 65504, bit 1 = NaN/Inf)")
    if collect is not None:
        collect.extend(preds)
    return stats


# ---------------------------------------------------------------------------------------------------
# real data, when the box has it (BASELINE configs[2]): TartanAir trajectory folder + reference checkpoint
# ---------------------------------------------------------------------------------------------------
def _read_rgb(path: str) -> np.ndarray:
    """PNG -> [3,H,W] float32 0..255 (what evaluate_stereo.py:150-157 hands the model: read_gen + permute + float)."""
    from PIL import Image
    with Image.open(path) as im:
        a = np.asarray(im.convert("RGB"), dtype=np.uint8)
    return np.ascontiguousarray(a.transpose(2, 0, 1)).astype(np.float32)


def load_tartanair_sequence(root: str, max_frames: Optional[int] = None, start: int = 0):
    """One TartanAir trajectory folder (e.g. .../abandonedfactory/Easy/P000) -> `synth.Sequence`.

    Layout and pairing follow the reference's temporal loader (core/stereo_datasets.py:491-495): sorted
    `image_left/*_left.png`, `image_right/*_right.png`, `depth_left/*_left_depth.npy`, and `pose_left.txt` with one
    pose per frame; disparity = 80 / (depth + 1e-5) (frame_utils.py:163-167); intrinsics and baseline are TartanAir's
    constants (evaluate_stereo.py:138-142).  Returns None (with the reason in `load_tartanair_sequence.why`) when the
    folder is absent or incomplete: callers then skip BASELINE configs[2] with that logged reason."""
    import glob
    import os

    from . import formats, synth

    def miss(why):
        load_tartanair_sequence.why = why
        return None

    if not root or not os.path.isdir(root):
        return miss(f"{root!r} is not a directory")
    left = sorted(glob.glob(os.path.join(root, "image_left", "*_left.png")))
    right = sorted(glob.glob(os.path.join(root, "image_right", "*_right.png")))
    depth = sorted(glob.glob(os.path.join(root, "depth_left", "*_left_depth.npy")))
    pose_file = os.path.join(root, "pose_left.txt")
    if not left or len(left) != len(right) or len(left) != len(depth) or not os.path.exists(pose_file):
        return miss(f"{root}: {len(left)} left / {len(right)} right / {len(depth)} depth files, pose_left.txt "
                    f"{'present' if os.path.exists(pose_file) else 'missing'}")
    poses = formats.read_tartanair_extrinsic(pose_file)
    if len(poses) < len(left):
        return miss(f"{root}: {len(poses)} poses for {len(left)} frames")
    stop = len(left) if max_frames is None else min(len(left), start + max_frames)
    frames = []
    for i in range(start, stop):
        disp, _valid = formats.read_disp_tartanair(depth[i])
        frames.append(synth.Frame(_read_rgb(left[i]), _read_rgb(right[i]), np.asarray(disp, np.float32)[None],
                                  np.asarray(poses[i], np.float32)))
    load_tartanair_sequence.why = ""
    return synth.Sequence(frames, synth.TARTANAIR_K.astype(np.float32), synth.TARTANAIR_BASELINE)


load_tartanair_sequence.why = ""


def load_checkpoint(model, path: str) -> int:
    """The reference's `.pth` (evaluate_stereo.py:385-390: `checkpoint['model']`, saved from DataParallel/DDP so keys may
    carry a `module.` prefix) into `model` with strict=True.  Only a weights-only load is attempted: a file that needs
    unpickling of arbitrary objects is refused rather than executed.  Returns the number of tensors loaded."""
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    state = ckpt["model"] if isinstance(ckpt, dict) and "model" in ckpt else ckpt
    state = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state.items()}
    model.load_state_dict(state, strict=True)
    return len(state)
