"""Grouped convolution launches: `with grouped(): a = conv2d(...); b = conv2d(...)` records the launches made inside the block and
issues them in pairs at its end through the library's `..._group` entry point, which runs a pair as one launch where it has a pair
kernel for the two tile instances and otherwise one after the other.  Shared by the fp32-tensor convolutions (ops.grouped,
tcs_conv2d_group) and the S16 ones (s16.grouped, tcs_conv2d_s16_group); each family records on its own.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

from . import native as nv


class Family:
    """One convolution entry point with its grouped counterparts (names in the library), and the block being recorded for it."""

    def __init__(self, prefix: str, desc_type, single: str, group: str, group_fused: str):
        self.prefix, self.desc_type, self.single, self.group, self.group_fused = prefix, desc_type, single, group, group_fused
        self.recording: Optional[list] = None       # (descriptor, name, objects its pointers refer to) of the open block

    def launch(self, d, name: str, keep: tuple):
        """The single launch now, or at the end of the enclosing `grouped()` block; `keep`: the objects whose memory `d` points to."""
        if self.recording is not None:
            self.recording.append((d, name, keep))
        else:
            nv.check(getattr(nv.lib(), self.single)(C.byref(d), nv.stream()), name)


class Grouped:
    """Context manager of one family (`family`, set by the subclass).  A recorded descriptor holds raw pointers only, so the block
    keeps every object the call was given (temporaries included) alive until the launch.  Blocks of one family do not nest."""
    family: Family

    def __init__(self, report: bool = False):
        self.report = report
        self.fused: List[bool] = []          # with `report`: per pair, whether the library issued it as one launch

    def __enter__(self):
        f = self.family
        if f.recording is not None:
            raise RuntimeError(f"{f.prefix}.grouped() does not nest")
        f.recording = []
        return self

    def __exit__(self, et, ev, tb):
        f = self.family
        descs, f.recording = f.recording, None
        if et is not None or not descs:
            return False
        lib = nv.lib()
        for i in range(0, len(descs), 2):
            chunk = descs[i:i + 2]
            arr = (C.POINTER(f.desc_type) * len(chunk))(*[C.pointer(d) for d, _, _ in chunk])
            if self.report:
                self.fused.append(len(chunk) == 2 and bool(getattr(lib, f.group_fused)(arr, 2)))
            nv.check(getattr(lib, f.group)(arr, len(chunk), nv.stream()), f.group + "[" + " | ".join(n for _, n, _ in chunk) + "]")
        return False
