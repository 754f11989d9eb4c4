#!/usr/bin/env python3
"""Cost of TCStereo.forward(test_mode=False) (every iteration's predictions, the cost volume, flow_mono / flow_init) against
test_mode=True, on one GPU.

bench.py's model and synthetic clips at 640x480 (seed 2000) and at the KITTI shape (375x1242, padded to 384x1248, seed 2100), 32
iterations, HIP graphs, no prefetch.  One model, both modes in this process, legs alternating (--rounds of --steps frames each; the clip
cycles, so 9 of every 10 frames run the temporal warp).  A test_mode=False step includes cloning its outputs out of the graph (about
2 * iters upsampled maps).  Prints one JSON line: ms per frame (min / median / max over all timed frames) per mode and shape, and the
median cost.

    python tools/bench_train_outputs.py [--steps 10] [--rounds 4] [--warmup 3] [--shapes 480x640,375x1242]

Each shape runs in a fresh child process (one shape: in this process), so no captured graph is dropped and re-captured in between.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (puts the package on the path)
import torch  # noqa: E402

MODES = ("test_mode", "train_outputs")


class Runner(bench.ClipRunner):
    """bench.ClipRunner with the call's test_mode chosen (the carried state is the same in both modes)."""

    def __init__(self, model, seq, dev, iters, test_mode):
        super().__init__(model, [seq], dev, iters, prefetch=False)
        self.test_mode = test_mode

    def step(self):
        i1, i2, K, T = self.frames[self.t]
        params = None
        if self.t > 0 and self.state is not None:
            flow_q, nets, fmap1, prev_T = self.state
            params = dict(K=K, T=T, previous_T=prev_T, last_disp=flow_q, last_net_list=nets, fmap1=fmap1, baseline=self.baseline)
        out = self.model(i1, i2, iters=self.iters, test_mode=self.test_mode, params=params)
        self.state = (out["flow_q"], out["net_list"], out["fmap1"], T)
        self.t = (self.t + 1) % self.n
        if self.t == 0:
            self.state = None
        return out


def time_frames(runner, steps):
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    for i in range(steps):
        marks[i].record()
        runner.step()
    marks[-1].record()
    torch.cuda.synchronize()
    return [marks[i].elapsed_time(marks[i + 1]) for i in range(steps)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="frames per timed leg")
    ap.add_argument("--rounds", type=int, default=4, help="legs per mode, alternating")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=bench.ITERS)
    ap.add_argument("--shapes", default="480x640,375x1242", help="HxW list")
    a = ap.parse_args()
    shapes = a.shapes.split(",")
    if len(shapes) > 1:
        res = None
        for shape in shapes:
            cmd = [sys.executable, "-X", "faulthandler", os.path.abspath(__file__), "--steps", str(a.steps), "--rounds", str(a.rounds),
                   "--warmup", str(a.warmup), "--iters", str(a.iters), "--shapes", shape]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if p.returncode != 0:
                print(f"[bench_train_outputs] {shape}: child exited with {p.returncode}", file=sys.stderr, flush=True)
                sys.exit(1)
            r = json.loads(p.stdout.strip().splitlines()[-1])
            res = r if res is None else dict(res, shapes={**res["shapes"], **r["shapes"]})
        print(json.dumps(res))
        return
    from tcs_mi355 import native, s16, synth
    native.lib()
    dev = torch.device("cuda:0")
    model, _ = bench.build_model(dev)
    model.use_hip_graph = True
    model._pipeline().strict = True
    res = {"metric": f"ms per frame, {a.iters} iterations, forward() with HIP graphs, test_mode=True vs test_mode=False (synthetic clip, "
                     f"cycling: 9 of 10 frames temporal)", "device": torch.cuda.get_device_name(dev), "steps": a.steps, "rounds": a.rounds,
           "shapes": {}}
    with torch.no_grad():
        for shape in shapes:
            h, w = (int(v) for v in shape.lower().split("x"))
            kitti = (h, w) == (375, 1242)
            seq = synth.make_sequence(2100 if kitti else 2000, n_frames=bench.CLIP_LEN, height=h, width=w, max_disp=bench.MAX_DISP,
                                      **(dict(K=synth.KITTI_K, baseline=0.54) if kitti else {}))
            runners = {m: Runner(model, seq, dev, a.iters, test_mode=(m == "test_mode")) for m in MODES}
            for m in MODES:
                for _ in range(max(a.warmup, 2)):
                    runners[m].step()
            s16.take_flags()
            times = {m: [] for m in MODES}
            for _ in range(a.rounds):
                for m in MODES:
                    times[m] += time_frames(runners[m], a.steps)
            r = {"domain_flags": s16.take_flags()}
            for m in MODES:
                t = sorted(times[m])
                r[m] = {"min": round(t[0], 3), "median": round(t[len(t) // 2], 3), "max": round(t[-1], 3)}
                print(f"[bench_train_outputs] {shape} {m}: {r[m]}", file=sys.stderr, flush=True)
            r["cost_ms_median"] = round(r["train_outputs"]["median"] - r["test_mode"]["median"], 3)
            r["cost_pct_median"] = round(100 * r["cost_ms_median"] / r["test_mode"]["median"], 2)
            res["shapes"][shape] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
