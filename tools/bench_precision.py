#!/usr/bin/env python3
"""Cost and accuracy of the fp16 precision mode (TCStereo hip_precision="fp16") against the default fp32 mode, on one GPU.

bench.py's model and synthetic clip (bench.build_model, 640x480, seed 2000), the drop-in call sequence (forward() only, HIP graphs, no
prefetch), both modes in this process, legs interleaved per iteration count: 32 iterations (BASELINE config 2) and 5 (the shipped eval
scripts' --valid_iters).  Prints one JSON line: ms per frame (min / median / max over the timed frames) per mode and leg, the EPE of the
fp16 mode's frame-0 output against the fp32 mode's and against the fp32 CPU oracle, and the domain flags of each mode's timed frames.

    python tools/bench_precision.py [--steps 20] [--warmup 3] [--no-oracle]
"""
import argparse
import json
import os
import sys
import time
from argparse import Namespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (puts the package on the path)
import torch  # noqa: E402


def models(dev):
    from core.tc_stereo import TCStereo
    m32, W = bench.build_model(dev)
    m16 = TCStereo(Namespace(**{**vars(m32.args), "hip_precision": "fp16"}))
    m16.load_state_dict(W, strict=True)
    m16 = m16.to(dev).eval()
    assert m32.hip_precision == "fp32" and m16.hip_precision == "fp16"
    return {"fp32": m32, "fp16": m16}, W


def time_leg(model, seq, dev, iters, steps, warmup):
    from tcs_mi355 import s16
    model.use_hip_graph = True
    runner = bench.ClipRunner(model, [seq], dev, iters, prefetch=False)
    for _ in range(max(warmup, 2)):
        runner.step()
    s16.take_flags()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    for i in range(steps):
        marks[i].record()
        runner.step()
    marks[-1].record()
    torch.cuda.synchronize()
    ms = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(steps))
    flags = s16.take_flags()
    return {"min": round(ms[0], 3), "median": round(ms[len(ms) // 2], 3), "max": round(ms[-1], 3)}, flags


def frame0(model, seq, dev, iters):
    runner = bench.ClipRunner(model, [seq], dev, iters, prefetch=False)
    out = runner.step()
    return {k: out[k].detach().cpu().double() for k in ("flow", "flow_q")}


def epe(a, b):
    return float((a - b).abs().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-oracle", action="store_true")
    a = ap.parse_args()
    from tcs_mi355 import native, synth
    native.lib()
    dev = torch.device("cuda:0")
    ms, W = models(dev)
    seq = synth.make_sequence(2000, n_frames=bench.CLIP_LEN, height=bench.HEIGHT, width=bench.WIDTH, max_disp=bench.MAX_DISP)
    res = {"metric": "ms per frame, 640x480, drop-in forward() with HIP graphs (frames 0-9 of the synthetic clip, cycling)",
           "device": torch.cuda.get_device_name(dev), "steps": a.steps, "legs": {}}
    with torch.no_grad():
        for iters in (32, 5):
            leg = {}
            for mode in ("fp32", "fp16"):
                t, flags = time_leg(ms[mode], seq, dev, iters, a.steps, a.warmup)
                leg[mode] = {"ms_per_frame": t, "domain_flags": flags}
                print(f"[bench_precision] iters={iters} {mode}: {t}", file=sys.stderr, flush=True)
            o32, o16 = frame0(ms["fp32"], seq, dev, iters), frame0(ms["fp16"], seq, dev, iters)
            leg["speedup_median"] = round(leg["fp32"]["ms_per_frame"]["median"] / leg["fp16"]["ms_per_frame"]["median"], 4)
            leg["frame0_epe_fp16_vs_fp32"] = {k: epe(o16[k], o32[k]) for k in o32}
            if not a.no_oracle:
                sys.path.insert(0, os.path.join(ROOT, "oracle"))
                import tcs_oracle as oracle
                fr = seq.frames[0]
                t0 = time.time()
                ref = oracle.tc_stereo_forward(W, torch.as_tensor(fr.image1)[None], torch.as_tensor(fr.image2)[None], iters=iters)
                leg["frame0_epe_vs_fp32_oracle"] = {m: {k: epe(o[k], ref[k].double()) for k in ("flow", "flow_q")}
                                                    for m, o in (("fp32", o32), ("fp16", o16))}
                print(f"[bench_precision] oracle {iters} iters: {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
            res["legs"][str(iters)] = leg
    print(json.dumps(res))


if __name__ == "__main__":
    main()
