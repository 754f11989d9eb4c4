#!/usr/bin/env python3
"""Cost of the deterministic mode (TCStereo hip_deterministic=True: the ordered splat) against the default float-atomic splat, on one GPU.

bench.py's model and synthetic clip (bench.build_model, 640x480, seed 2000, 32 iterations), the drop-in call sequence (forward() only, HIP
graphs, no prefetch), both modes in this process, legs alternating (--rounds of --steps frames each; the clip cycles, so 9 of every 10
frames run the temporal warp).  Prints one JSON line: ms per frame (min / median / max over all timed frames) per mode, the per-frame EPE
between the modes over one free run of the clip, whether each mode reproduces itself bit for bit over a second run, and the domain flags.

    python tools/bench_deterministic.py [--steps 10] [--rounds 4] [--warmup 3]
"""
import argparse
import json
import os
import sys
from argparse import Namespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (puts the package on the path)
import torch  # noqa: E402

MODES = ("default", "deterministic")


def models(dev):
    from core.tc_stereo import TCStereo
    m0, W = bench.build_model(dev)
    m1 = TCStereo(Namespace(**{**vars(m0.args), "hip_deterministic": True}))
    m1.load_state_dict(W, strict=True)
    m1 = m1.to(dev).eval()
    assert not m0.hip_deterministic and m1.hip_deterministic
    return {"default": m0, "deterministic": m1}


def time_frames(runner, steps):
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    for i in range(steps):
        marks[i].record()
        runner.step()
    marks[-1].record()
    torch.cuda.synchronize()
    return [marks[i].elapsed_time(marks[i + 1]) for i in range(steps)]


def clip_flows(model, seq, dev, iters):
    runner = bench.ClipRunner(model, [seq], dev, iters, prefetch=False)
    return [runner.step()["flow"].detach().clone() for _ in range(len(seq.frames))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="frames per timed leg")
    ap.add_argument("--rounds", type=int, default=4, help="legs per mode, alternating")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=bench.ITERS)
    a = ap.parse_args()
    from tcs_mi355 import native, s16, synth
    native.lib()
    dev = torch.device("cuda:0")
    ms = models(dev)
    seq = synth.make_sequence(2000, n_frames=bench.CLIP_LEN, height=bench.HEIGHT, width=bench.WIDTH, max_disp=bench.MAX_DISP)
    res = {"metric": f"ms per frame, 640x480, {a.iters} iterations, drop-in forward() with HIP graphs (synthetic clip, cycling: 9 of 10 "
                     f"frames temporal)", "device": torch.cuda.get_device_name(dev), "steps": a.steps, "rounds": a.rounds, "modes": {}}
    with torch.no_grad():
        runners = {}
        for mode in MODES:
            ms[mode].use_hip_graph = True
            runners[mode] = bench.ClipRunner(ms[mode], [seq], dev, a.iters, prefetch=False)
            for _ in range(max(a.warmup, 2)):
                runners[mode].step()
        s16.take_flags()
        times = {m: [] for m in MODES}
        flags = {m: 0 for m in MODES}
        for _ in range(a.rounds):
            for mode in MODES:
                times[mode] += time_frames(runners[mode], a.steps)
                flags[mode] |= s16.take_flags()
        for mode in MODES:
            t = sorted(times[mode])
            res["modes"][mode] = {"ms_per_frame": {"min": round(t[0], 3), "median": round(t[len(t) // 2], 3), "max": round(t[-1], 3)},
                                  "domain_flags": flags[mode]}
            print(f"[bench_deterministic] {mode}: {res['modes'][mode]['ms_per_frame']}", file=sys.stderr, flush=True)
        res["cost_ms_median"] = round(res["modes"]["deterministic"]["ms_per_frame"]["median"] -
                                      res["modes"]["default"]["ms_per_frame"]["median"], 3)
        runs = {m: [clip_flows(ms[m], seq, dev, a.iters) for _ in range(2)] for m in MODES}
        res["epe_per_frame_deterministic_vs_default"] = [float((x - y).abs().mean()) for x, y in
                                                         zip(runs["deterministic"][0], runs["default"][0])]
        res["bit_reproducible_over_two_runs"] = {m: all(torch.equal(x, y) for x, y in zip(*runs[m])) for m in MODES}
        res["epe_per_frame_run_to_run"] = {m: [float((x - y).abs().mean()) for x, y in zip(*runs[m])] for m in MODES}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
