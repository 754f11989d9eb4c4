#!/usr/bin/env python3
"""Mixed batches (params["new_sequence"]) on one GPU: bench.py's model (bench.build_model, HIP graphs, the float-atomic splat).

(a) overhead: 4 lock-step synthetic 640x480 clips at --iters iterations, the temporal path against the mixed path with an all-False
    mask (the prior copy and the whole-batch arg-max on every frame), legs alternating (--rounds of --steps frames each; the clips
    cycle, so 9 of every 10 frames are temporal), median ms per step of 4 pairs.
(b) continuous batching: --seqs synthetic 640x480 sequences of 3..10 frames, `run_sequence` one by one against
    `run_sequences(batch=--batch)`, stereo pairs per second over the whole set (padding not counted), and the largest per-frame EPE
    between the two runs' predictions and the largest per-sequence difference of the EPE against ground truth.
Prints one JSON line.  `--only b` runs (b) alone (for a kernel trace of it); `--deterministic` uses the ordered splat, so that the
EPE between the runs shows what batching changes and not the float-atomic splat's run-to-run differences, which the recurrence
amplifies over a sequence.

    python tools/bench_mixed_batch.py [--steps 10] [--rounds 4] [--warmup 3] [--seqs 8] [--batch 4] [--only a|b]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (puts the package on the path)
import torch  # noqa: E402

LANES = 4


class MixedRunner(bench.ClipRunner):
    """bench.ClipRunner whose temporal frames carry params["new_sequence"] = all False (the mixed path, same results)."""

    def step(self):
        model = self.model
        mask = self.mask

        class Wrap:
            def __call__(self, *a, params=None, **kw):
                if params is not None:
                    params = dict(params, new_sequence=mask)
                return model(*a, params=params, **kw)

        self.model = Wrap()
        try:
            return super().step()
        finally:
            self.model = model


def time_steps(runner, steps):
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    for i in range(steps):
        marks[i].record()
        runner.step()
    marks[-1].record()
    torch.cuda.synchronize()
    return [marks[i].elapsed_time(marks[i + 1]) for i in range(steps)]


def overhead(model, dev, a):
    from tcs_mi355 import synth
    seqs = [synth.make_sequence(2000 + j, n_frames=bench.CLIP_LEN, height=bench.HEIGHT, width=bench.WIDTH, max_disp=bench.MAX_DISP)
            for j in range(LANES)]
    runners = {"temporal": bench.ClipRunner(model, seqs, dev, a.iters, prefetch=False),
               "mixed_all_false": MixedRunner(model, seqs, dev, a.iters, prefetch=False)}
    runners["mixed_all_false"].mask = torch.zeros(LANES, dtype=torch.bool, device=dev)
    for r in runners.values():
        for _ in range(max(a.warmup, 2)):
            r.step()
    times = {k: [] for k in runners}
    for _ in range(a.rounds):
        for k, r in runners.items():
            times[k] += time_steps(r, a.steps)
    res = {}
    for k, t in times.items():
        t = sorted(t)
        res[k] = {"min": round(t[0], 3), "median": round(t[len(t) // 2], 3), "max": round(t[-1], 3)}
        print(f"[bench_mixed_batch] (a) {k}: {res[k]}", file=sys.stderr, flush=True)
    res["overhead_ms_median"] = round(res["mixed_all_false"]["median"] - res["temporal"]["median"], 3)
    return res


def continuous(model, dev, a):
    from tcs_mi355 import synth
    from tcs_mi355.harness import run_sequence, run_sequences
    lengths = [3 + (7 * j) // max(a.seqs - 1, 1) for j in range(a.seqs)]           # 3..10 frames
    data = [synth.make_sequence(3000 + j, n_frames=n, height=bench.HEIGHT, width=bench.WIDTH, max_disp=bench.MAX_DISP)
            for j, n in enumerate(lengths)]
    frames = sum(lengths)
    # warm-up: every graph both paths need (first / temporal at batch 1; first / mixed / temporal at batch --batch)
    run_sequence(model, data[0], iters=a.iters, device=dev)
    run_sequences(model, data[:a.batch + 1], iters=a.iters, device=dev, batch=a.batch)
    torch.cuda.synchronize()
    single, batched = [], []
    t0 = time.perf_counter()
    s_stats = []
    for q in data:
        c = []
        s_stats.append(run_sequence(model, q, iters=a.iters, device=dev, collect=c))
        single.append(c)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    b_stats = run_sequences(model, data, iters=a.iters, device=dev, batch=a.batch, collect=batched)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    epe = max(float((x - y).abs().mean()) for s, b in zip(single, batched) for x, y in zip(s, b))
    seq_epe = max(abs(float(s.vector()[0] / max(len(s.frames), 1)) - float(b.vector()[0] / max(len(b.frames), 1)))
                  for s, b in zip(s_stats, b_stats))
    res = {"lengths": lengths, "frames": frames, "batch": a.batch,
           "run_sequence_pairs_per_s": round(frames / (t1 - t0), 2), "run_sequences_pairs_per_s": round(frames / (t2 - t1), 2),
           "max_frame_epe_between_runs": epe, "max_sequence_epe_vs_gt_difference": seq_epe,
           "domain_flags": int(b_stats[0].domain_flags) if b_stats else 0}
    print(f"[bench_mixed_batch] (b) {res}", file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="steps per timed leg of (a)")
    ap.add_argument("--rounds", type=int, default=4, help="legs per path in (a), alternating")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=bench.ITERS)
    ap.add_argument("--seqs", type=int, default=8)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--only", choices=("a", "b"), default=None)
    ap.add_argument("--deterministic", action="store_true", help="the model with hip_deterministic=True (the ordered splat)")
    a = ap.parse_args()
    from tcs_mi355 import native
    native.lib()
    dev = torch.device("cuda:0")
    model, weights = bench.build_model(dev)
    if a.deterministic:
        from argparse import Namespace

        from core.tc_stereo import TCStereo
        model = TCStereo(Namespace(**{**vars(model.args), "hip_deterministic": True}))
        model.load_state_dict(weights, strict=True)
        model = model.to(dev).eval()
    model.use_hip_graph = True
    splat = "ordered splat (hip_deterministic)" if a.deterministic else "float-atomic splat"
    res = {"metric": f"640x480, {a.iters} iterations, HIP graphs, {splat}", "device": torch.cuda.get_device_name(dev)}
    with torch.no_grad():
        if a.only in (None, "a"):
            res["a_lockstep_4_ms_per_step"] = overhead(model, dev, a)
        if a.only in (None, "b"):
            res["b_continuous"] = continuous(model, dev, a)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
