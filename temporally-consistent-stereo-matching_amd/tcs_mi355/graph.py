"""A TC-Stereo frame as a two-stage pipeline, replayed from HIP graphs.

A frame has two parts.  EXTRACT — image normalisation, feature / context networks, correlation pyramid, context convolutions
(core/tc_stereo.py:101-116,147-149 of the reference) — depends on nothing but the two images.  REFINE — the temporal warp or
arg-max prior, disparity completion, hidden-state warp and the refinement loop (tc_stereo.py:119-229) — needs EXTRACT's
features and the previous frame's outputs.  Both stages are enqueued on the caller's stream and run back to back, as in the
reference.  A caller that knows its next frame may enqueue that frame's EXTRACT early: `prefetch(image1, image2)` launches it,
behind the frame in flight, into the free one of two feature slots, and the following `__call__` with the same image tensors
finds it there.  What that buys, as measured (profiles/r03_frame_phases.txt): the HOST-side launch work of
the next EXTRACT (0.35-0.6 ms per frame) leaves the frame's serial path.  On the GPU the extraction still runs after the loop.

A `test_mode=False` frame (`outputs=True`: every iteration's predictions, the cost volume) is its own EXTRACT key (the build also writes
the cost volume) and its own REFINE key (the loop's outputs mode); features prefetched for a test-mode frame are not consumed by it.

Each stage is ~100 / ~1,700 kernel launches with static shapes and no host decision inside, so it is captured once per
(shape, branch[, iteration count]) and slot into a HIP graph and replayed.  Inputs are copied into the graph's static
buffers, outputs are cloned out, so callers keep ordinary tensor semantics (the temporal state they pass back next frame
is theirs).  The library kernels are capture-safe by construction (no allocation, no sync — include/tcs_mi355.h).
Two slots also give two executables per stage, used in turn: on ROCm 7.2 launching an executable graph WITH parallel
branches again blocks the host until its previous launch has nearly finished (tools/capture_variance.py), and alternating
lets the host enqueue frame t+1 while frame t runs.
"""
from __future__ import annotations

import gc
import warnings
from typing import Callable, Dict, List, Optional

import torch

_CAPTURING = 0          # > 0 while any FrameGraphs capture is recording (FrameGraphs.drop refuses then)


# what the loop's outputs mode adds to the frame's dict (TCStereo._refine_loop(outputs=True))
_OUTPUTS_KEYS = ("up", "q", "grad", "flow_mono", "flow_init", "cost_volume")


def _flatten(temporal):
    """A mixed batch's temporal tuple has an 8th entry, the uint8 [B] sequence-start mask: one more static input of REFINE."""
    if temporal is None:
        return []
    K, T, Tp, base, last_disp, nets, fmap1 = temporal[:7]
    return [K, T, Tp, base, last_disp, *nets, fmap1, *temporal[7:]]


def _unflatten(flat):
    if not flat:
        return None
    if flat[-1].dtype == torch.uint8:
        return _unflatten(flat[:-1]) + (flat[-1],)
    return (flat[0], flat[1], flat[2], flat[3], flat[4], list(flat[5:-1]), flat[-1])


def _wants_argmax(temporal):
    """A first frame and every frame of a mixed batch consume an EXTRACT made with the arg-max prior (the `first=True` extract key)."""
    return temporal is None or len(temporal) == 8


class _no_gc:
    """No cyclic garbage collection while a stream is capturing.  torch.cuda.graph() collects before it starts capturing; a collection that
    fires DURING the capture and finds an unreachable HIP graph / event of an earlier capture destroys it mid-capture, and the runtime aborts
    the process (seen once: `Fatal Python error: Aborted ... Garbage-collecting` inside `_capture_extract` after a weight change had dropped
    the previous captures)."""

    def __enter__(self):
        global _CAPTURING
        self.was = gc.isenabled()
        gc.disable()
        _CAPTURING += 1

    def __exit__(self, *exc):
        global _CAPTURING
        _CAPTURING -= 1
        if self.was:
            gc.enable()
        return False


class _Slot:
    """One of the two feature slots: what the last EXTRACT into it produced, and for which images."""

    def __init__(self):
        self.feats = None
        self.token = None                      # identifies the images (and mode) the features belong to
        self.fresh = False                     # features nobody has consumed yet
        self.by_prefetch = False
        self.age = 0                           # calls since the features were produced without anybody consuming them
        self.ex_key = None


class _Entry:
    """A captured stage: its graph (REFINE: the head; `graph2` the loop, and `start` the head's outputs, which the loop graph holds
    raw pointers to), the static inputs it reads and the outputs it writes."""

    def __init__(self, graph, static_in, static_out, graph2=None, start=None):
        self.graph, self.static_in, self.static_out, self.graph2, self.start = graph, static_in, static_out, graph2, start


class FrameGraphs:
    """`extract_fn(image1, image2, first, outputs) -> feats`, `head_fn(feats, temporal) -> start`, `loop_fn(feats, start, iters, outputs)
    -> dict` (`outputs`: a test_mode=False frame).
    REFINE is captured as two graphs, the short state-dependent head and the loop, replayed back to back.

    `epoch_fn` returns a value that changes whenever a model parameter is replaced or written in place (`load_state_dict`, an
    optimiser step): a captured graph holds the packed weight images of the moment of capture, so every entry is dropped and
    re-captured when it changes.  `fell_back` counts the frames that ran eagerly because a capture failed; `strict=True` turns
    such a failure into an error instead (bench.py, tests).  `captures` counts captured REFINE keys."""

    def __init__(self, extract_fn: Callable, head_fn: Callable, loop_fn: Callable, warmup: int = 2,
                 epoch_fn: Optional[Callable[[], object]] = None, strict: bool = False):
        self.extract_fn, self.head_fn, self.loop_fn = extract_fn, head_fn, loop_fn
        self.warmup, self.epoch_fn, self.strict = warmup, epoch_fn, strict
        self.slots = [_Slot(), _Slot()]
        self.turn = 0                          # the slot the next EXTRACT goes to (unless it still holds unconsumed features)
        self.ex: Dict[tuple, Optional[List[_Entry]]] = {}
        self.rf: Dict[tuple, Optional[List[_Entry]]] = {}
        self.epoch = epoch_fn() if epoch_fn is not None else None
        self.fell_back = 0
        self.captures = 0
        self.prefetched = 0                    # frames whose EXTRACT had been launched by prefetch()

    # ---- bookkeeping ---------------------------------------------------------------------------------------------------------
    @property
    def cache(self):
        return {**{("extract", *k): v for k, v in self.ex.items()}, **{("refine", *k): v for k, v in self.rf.items()}}

    def _check_epoch(self):
        if self.epoch_fn is not None:
            now = self.epoch_fn()
            if now != self.epoch:              # weights changed: the captured packed-weight images are stale
                torch.cuda.synchronize()
                self.ex.clear()
                self.rf.clear()
                self.slots = [_Slot(), _Slot()]
                self.turn, self.epoch = 0, now
                gc.collect()                   # the dropped captures die here, not inside the next capture (see _no_gc)

    def drop(self):
        """Release every captured graph NOW (e.g. between two benchmark legs).  Destroying a HIP graph while another stream is recording a
        capture aborts the process on ROCm 7.2 (the round-3 abort came through the garbage collector; `del` / `= None` of a FrameGraphs
        or of its entries is the same thing by hand), so this refuses while any capture is active, waits for the device, drops the
        entries and collects at once."""
        if _CAPTURING:
            raise RuntimeError("FrameGraphs.drop() while a HIP graph capture is recording")
        torch.cuda.synchronize()
        self.ex.clear()
        self.rf.clear()
        self.slots = [_Slot(), _Slot()]
        self.turn = 0
        gc.collect()

    def _pick_slot(self) -> int:
        """Where the next EXTRACT goes: the slot whose features have been consumed (a prefetch made for the NEXT frame must survive
        the call for the current one); with two unconsumed sets, the older.  A prefetch nobody consumed ages out (`__call__`): after
        two calls that did not match it the slot is free again and its image tensors are released — one mispredicted prefetch must not
        pin a slot (and with it the two-executable alternation) for the rest of the process."""
        for k in (self.turn, self.turn ^ 1):
            if not self.slots[k].fresh:
                return k
        return self.turn

    @staticmethod
    def _token(image1, image2, first, use_graph, outputs=False):
        """Identifies the frame a slot's features belong to: the image tensor OBJECTS (the slot keeps them alive, so their storage
        cannot be handed to other tensors meanwhile — a data_ptr alone can come back with other content), their versions (no
        in-place write since), the branch, the launch mode and whether the features include the cost volume (`outputs`)."""
        return (image1, image1._version, image2, image2._version, bool(first), bool(use_graph), bool(outputs))

    @staticmethod
    def _same(a, b):
        return a is not None and b is not None and a[0] is b[0] and a[2] is b[2] and a[1] == b[1] and a[3] == b[3] and a[4:] == b[4:]

    @staticmethod
    def _ex_key(image1, first, outputs=False):
        return (tuple(image1.shape), image1.device.index, bool(first), bool(outputs))

    @staticmethod
    def _rf_key(image1, iters, flat, outputs=False):
        return (tuple(image1.shape), image1.device.index, int(iters), tuple(tuple(t.shape) for t in flat), bool(outputs))

    # ---- EXTRACT -------------------------------------------------------------------------------------------------------------
    def _capture_extract(self, key, image1, image2, first, outputs=False) -> Optional[List[_Entry]]:
        static_in = [image1.clone(), image2.clone()]
        run = lambda: self.extract_fn(static_in[0], static_in[1], first, outputs)
        # The warm-up and the capture write the model's pool buffers, which every extract key of this shape shares: whatever a slot
        # holds unconsumed is no longer trustworthy.
        for sl in self.slots:
            sl.fresh, sl.token = False, None
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(self.warmup):        # packs weights, sizes the pools
                    run()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            entries = []
            for _ in range(2):                      # one executable (and one set of output tensors) per slot
                g = torch.cuda.CUDAGraph()
                with _no_gc(), torch.cuda.graph(g):
                    feats = run()
                g.replay()          # the first launch of an executable graph uploads it (~30 ms): pay that here, not in a timed frame
                entries.append(_Entry(g, static_in, feats))
            torch.cuda.synchronize()
            return entries
        except Exception as e:  # capture is an optimisation: the eager HIP path computes the same thing
            if self.strict:
                raise
            warnings.warn(f"HIP graph capture of the extract stage failed ({type(e).__name__}: {e}); running this shape with eager launches")
            torch.cuda.synchronize()
            return None

    def _launch_extract(self, si: int, image1, image2, first: bool, use_graph: bool, outputs: bool = False):
        """EXTRACT into slot `si` on the caller's stream, behind everything already queued there (the slot's last reader included)."""
        slot = self.slots[si]
        key = self._ex_key(image1, first, outputs)
        entries = None
        if use_graph:
            if key not in self.ex:
                self.ex[key] = self._capture_extract(key, image1, image2, first, outputs)
            entries = self.ex[key]
        if entries is not None:
            e = entries[si]
            e.static_in[0].copy_(image1)
            e.static_in[1].copy_(image2)
            e.graph.replay()
            slot.feats = e.static_out
        else:
            slot.feats = self.extract_fn(image1, image2, first, outputs)
        slot.token, slot.ex_key, slot.fresh, slot.by_prefetch, slot.age = self._token(image1, image2, first, use_graph, outputs), key, True, False, 0
        self.turn = si ^ 1

    def prefetch(self, image1, image2, first: bool = False, use_graph: bool = True) -> int:
        """Launch the EXTRACT stage of a coming frame; the next `__call__` with the same image tensor objects (unmodified) uses it.
        `first=True` for a frame that will be called with params=None OR as a mixed batch (params["new_sequence"] present, whatever
        its values): both consume the extract made with the arg-max prior.  A mixed frame does not pick up a `first=False` prefetch.
        Call it right after the `__call__` it follows.  Returns the slot."""
        self._check_epoch()
        token = self._token(image1, image2, first, use_graph)
        for k in (0, 1):
            if self.slots[k].fresh and self._same(self.slots[k].token, token):
                return k                                    # already there
        si = self._pick_slot()
        self._launch_extract(si, image1, image2, first, use_graph)
        self.slots[si].by_prefetch = True
        return si

    # ---- REFINE --------------------------------------------------------------------------------------------------------------
    def _capture_refine(self, key, image1, image2, iters, flat, first, outputs=False) -> Optional[List[_Entry]]:
        ex_key = self._ex_key(image1, first, outputs)
        try:
            for si in (0, 1):                        # both slots need features of this shape / branch to capture against
                if self.slots[si].feats is None or self.slots[si].ex_key != ex_key or self.ex.get(ex_key) is None \
                        or self.slots[si].feats is not self.ex[ex_key][si].static_out:
                    self._launch_extract(si, image1, image2, first, True, outputs=outputs)
            if self.ex.get(ex_key) is None:
                return None                          # the extract stage runs eagerly: so does this one
            torch.cuda.synchronize()
            static_in = [t.detach().clone() if t.dtype == torch.uint8 else t.detach().float().clone() for t in flat]
            entries = []
            for si in (0, 1):
                feats = self.ex[ex_key][si].static_out
                run = lambda: self.loop_fn(feats, self.head_fn(feats, _unflatten(static_in)), iters, outputs)
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for _ in range(self.warmup if si == 0 else 1):
                        run()
                torch.cuda.current_stream().wait_stream(side)
                torch.cuda.synchronize()
                g1, g2 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
                with _no_gc(), torch.cuda.graph(g1):
                    start = self.head_fn(feats, _unflatten(static_in))
                g1.replay()                               # (the loop graph is captured against the head graph's output tensors)
                with _no_gc(), torch.cuda.graph(g2):
                    out = self.loop_fn(feats, start, iters, outputs)
                g2.replay()
                entries.append(_Entry(g1, static_in, out, graph2=g2, start=start))
            torch.cuda.synchronize()
            self.captures += 1
            for sl in self.slots:                       # the capture used both slots: whatever was prefetched into them is gone
                sl.fresh, sl.token = False, None
            return entries
        except Exception as e:
            if self.strict:
                raise
            warnings.warn(f"HIP graph capture failed ({type(e).__name__}: {e}); running this shape with eager launches")
            torch.cuda.synchronize()
            return None

    def __call__(self, image1, image2, iters, temporal, use_graph: bool = True, outputs: bool = False):
        """One frame.  `outputs` (a test_mode=False call): the loop's outputs mode on features extracted with the cost volume; the
        returned dict then also holds the loop's stacked per-iteration tensors, flow_mono, flow_init and cost_volume, all cloned."""
        self._check_epoch()
        flat = _flatten(temporal)
        first = _wants_argmax(temporal)
        token = self._token(image1, image2, first, use_graph, outputs)
        entries = None
        if use_graph:
            key = self._rf_key(image1, iters, flat, outputs)
            if key not in self.rf:
                self.rf[key] = self._capture_refine(key, image1, image2, iters, flat, first, outputs)
            entries = self.rf[key]
            if entries is None:
                self.fell_back += 1
        si = next((k for k in (0, 1) if self.slots[k].fresh and self._same(self.slots[k].token, token)), None)
        for k in (0, 1):                                # unconsumed features this call does not match: one call older
            sl = self.slots[k]
            if sl.fresh and k != si:
                sl.age += 1
                if sl.age >= 2:
                    sl.fresh, sl.token = False, None
        if si is not None:
            self.prefetched += int(self.slots[si].by_prefetch)
        else:
            si = self._pick_slot()
            self._launch_extract(si, image1, image2, first, use_graph and entries is not None, outputs=outputs)
        slot = self.slots[si]
        slot.fresh, slot.token = False, None            # consumed (and the image tensors are no longer held)
        if entries is not None and self.ex.get(slot.ex_key) is not None and slot.feats is self.ex[slot.ex_key][si].static_out:
            e = entries[si]
            for dst, src in zip(e.static_in, flat):
                dst.copy_(src)
            e.graph.replay()                            # head
            e.graph2.replay()                           # loop
            o = e.static_out
            out = {"flow": o["flow"].clone(), "flow_q": o["flow_q"].clone(), "net_list": [t.clone() for t in o["net_list"]],
                   "fmap1": o["fmap1"].clone()}
            for k in _OUTPUTS_KEYS if outputs else ():
                out[k] = o[k].clone()
        else:
            start = self.head_fn(slot.feats, temporal)
            if outputs:
                out = self.loop_fn(slot.feats, start, iters, True)
                out = dict(out, fmap1=out["fmap1"].clone(), cost_volume=out["cost_volume"].clone())   # (both belong to the slot)
            else:
                out = self.loop_fn(slot.feats, start, iters)
                out = dict(out, fmap1=out["fmap1"].clone())      # the slot's tensor is overwritten two frames from now
        return out
