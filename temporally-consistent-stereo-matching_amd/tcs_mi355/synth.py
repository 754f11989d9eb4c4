"""Synthetic stereo sequences of the shapes BASELINE.json names.

A scene is a handful of textured planes seen by a rectified pinhole stereo rig that moves along a
smooth trajectory.  Left and right images are ray-cast analytically (so occlusions are right), the
texture is a band-limited sum of sinusoids in plane coordinates, images are uint8-quantised and
returned as float 0..255 like the reference loader does (evaluate_stereo.py:156-157).  Ground-truth
disparity is fx*baseline/Z of the left view and is bounded by `max_disp` ("D" of the metric — the
reference has no D parameter; 192 only appears as the GT validity bound, evaluate_stereo.py:205).
Poses are world->camera 4x4 matrices, the convention of read_tartanair_extrinsic
(core/utils/frame_utils.py:231-259) as consumed by cal_relative_transformation (geo_utils.py:148-155).

Everything is numpy with a Philox generator: the same sequence on every machine.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List

import numpy as np

TARTANAIR_K = np.array([[320.0, 0.0, 320.0], [0.0, 320.0, 240.0], [0.0, 0.0, 1.0]])   # stereo_datasets.py:521-523
TARTANAIR_BASELINE = 0.25                                                               # stereo_datasets.py:524
KITTI_K = np.array([[721.5377, 0.0, 609.5593], [0.0, 721.5377, 172.854], [0.0, 0.0, 1.0]])
KITTI_BASELINE = 0.54                                                                   # stereo_datasets.py:632


@dataclass
class Frame:
    image1: np.ndarray      # [3,H,W] float32, 0..255 (left)
    image2: np.ndarray      # [3,H,W] float32, 0..255 (right)
    disp_gt: np.ndarray     # [1,H,W] float32, positive disparity of the left view
    T: np.ndarray           # [4,4] float32 world->camera


@dataclass
class Sequence:
    frames: List[Frame]
    K: np.ndarray           # [3,3] float32 (full resolution)
    baseline: float


class _Plane:
    def __init__(self, gen, point, normal, n_waves=8, extent=None):
        self.extent = extent                      # half-size in plane coordinates, None = infinite
        self.p0 = np.asarray(point, np.float64)
        n = np.asarray(normal, np.float64)
        self.n = n / np.linalg.norm(n)
        a = np.cross(self.n, [0.0, 1.0, 0.0])
        if np.linalg.norm(a) < 1e-3:
            a = np.cross(self.n, [1.0, 0.0, 0.0])
        self.u = a / np.linalg.norm(a)
        self.v = np.cross(self.n, self.u)
        # band-limited texture: random directions, wavelengths 0.1 .. 1.6 m, per colour channel
        self.freq = gen.uniform(0.6, 10.0, size=(n_waves, 1)) * _unit2(gen, n_waves)
        self.phase = gen.uniform(0, 2 * np.pi, size=(3, n_waves))
        self.amp = gen.uniform(0.4, 1.0, size=(3, n_waves))
        self.amp /= self.amp.sum(1, keepdims=True)
        self.base = gen.uniform(90, 165, size=3)

    def intersect(self, origin, dirs):
        """Ray parameter t (>0 in front) for rays origin + t*dirs, dirs [...,3]."""
        denom = dirs @ self.n
        num = (self.p0 - origin) @ self.n
        with np.errstate(divide="ignore", invalid="ignore"):
            t = num / denom
        t = np.where(np.abs(denom) < 1e-9, np.inf, t)
        if self.extent is not None:
            ok = np.isfinite(t) & (t > 0)
            rel = origin + dirs * np.where(ok, t, 0.0)[..., None] - self.p0
            inside = (np.abs(rel @ self.u) < self.extent) & (np.abs(rel @ self.v) < self.extent)
            t = np.where(ok & inside, t, np.inf)
        return t

    def colour(self, pts):
        rel = pts - self.p0
        uv = np.stack([rel @ self.u, rel @ self.v], -1)                  # [...,2]
        arg = uv @ self.freq.T * (2 * np.pi)                            # [...,n_waves]
        tex = np.sin(arg[..., None, :] + self.phase) * self.amp         # [...,3,n_waves]
        return self.base + 110.0 * tex.sum(-1)


def _unit2(gen, n):
    a = gen.uniform(0, 2 * np.pi, size=n)
    return np.stack([np.cos(a), np.sin(a)], 1)


def _pose(t_idx, step, yaw_deg):
    """Camera-to-world: forward motion along +z with a slow yaw; returned as world->camera."""
    yaw = np.deg2rad(yaw_deg) * t_idx
    c, s = np.cos(yaw), np.sin(yaw)
    R_c2w = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    pos = np.array([0.02 * t_idx, 0.0, step * t_idx])
    T_c2w = np.eye(4)
    T_c2w[:3, :3] = R_c2w
    T_c2w[:3, 3] = pos
    return np.linalg.inv(T_c2w)


def _render(planes, T_w2c, K, h, w, cam_offset_x):
    """Ray-cast one view.  cam_offset_x shifts the camera centre along its own +x (right camera)."""
    T_c2w = np.linalg.inv(T_w2c)
    R, pos = T_c2w[:3, :3], T_c2w[:3, 3]
    origin = pos + R @ np.array([cam_offset_x, 0.0, 0.0])
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    dirs_c = np.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], np.ones_like(xs)], -1)
    dirs_w = dirs_c @ R.T
    best_t = np.full((h, w), np.inf)
    img = np.zeros((h, w, 3))
    for pl in planes:
        t = pl.intersect(origin, dirs_w)
        hit = (t > 1e-3) & (t < best_t)
        if not hit.any():
            continue
        pts = origin + dirs_w[hit] * t[hit][:, None]
        img[hit] = pl.colour(pts)
        best_t = np.where(hit, t, best_t)
    depth = best_t            # dirs_c has z = 1, so t IS the camera-frame depth
    return img, depth


def make_sequence(seed: int, n_frames: int = 10, height: int = 480, width: int = 640, max_disp: float = 192.0,
                  K: np.ndarray = TARTANAIR_K, baseline: float = TARTANAIR_BASELINE, step: float = 0.05,
                  yaw_deg: float = 0.5) -> Sequence:
    """Config 2 of BASELINE.json by default: 640x480, D=192, 10 frames, TartanAir intrinsics.
    `K` is scaled with the image size when height/width differ from 480x640 so the field of view is kept."""
    gen = np.random.Generator(np.random.Philox(key=int(seed)))
    K = np.array(K, np.float64)
    if (height, width) != (480, 640) and K is not KITTI_K and np.allclose(K, TARTANAIR_K):
        sx, sy = width / 640.0, height / 480.0
        K = K * np.array([[sx], [sy], [1.0]])
    fx = K[0, 0]
    z_min = fx * baseline / max_disp * 1.15        # keeps disparity < max_disp over the whole clip
    travel = step * (n_frames + 1)
    # a back wall, a slanted floor-ish plane, and 2-3 slanted foreground panels
    planes = [_Plane(gen, [0, 0, z_min * gen.uniform(9, 14) + travel], [gen.uniform(-.15, .15), gen.uniform(-.1, .1), -1])]
    # floor: low enough that its nearest visible point (bottom image row) stays beyond z_min
    y_floor = z_min * (height / 2.0) / K[1, 1] * gen.uniform(1.15, 1.6)
    planes.append(_Plane(gen, [0, y_floor, 0], [gen.uniform(-.05, .05), -1, gen.uniform(-.12, -.03)]))
    for _ in range(int(gen.integers(2, 4))):
        z = z_min * gen.uniform(1.6, 5.0) + travel
        planes.append(_Plane(gen, [gen.uniform(-1.2, 1.2) * z * 0.5, gen.uniform(-0.3, 0.2) * z * 0.5, z],
                             [gen.uniform(-.6, .6), gen.uniform(-.3, .3), -1], extent=z * gen.uniform(0.18, 0.4)))
    frames = []
    for t in range(n_frames):
        T = _pose(t, step, yaw_deg)
        left, depth = _render(planes, T, K, height, width, 0.0)
        right, _ = _render(planes, T, K, height, width, baseline)
        depth = np.maximum(depth, z_min)
        disp = fx * baseline / depth
        q = lambda im: np.clip(np.rint(im), 0, 255).astype(np.float32).transpose(2, 0, 1)
        frames.append(Frame(q(left), q(right), disp[None].astype(np.float32), T.astype(np.float32)))
    return Sequence(frames, K.astype(np.float32), float(baseline))


def make_pair(seed: int, height: int = 240, width: int = 320, max_disp: float = 64.0) -> Frame:
    """Config 1 of BASELINE.json: a single 320x240 pair, D=64."""
    return make_sequence(seed, n_frames=1, height=height, width=width, max_disp=max_disp).frames[0]


def make_loss_case(seed: int, B: int = 1, H: int = 32, W: int = 48, iters: int = 3, empty: bool = False) -> dict:
    """Inputs of the training objective (train_stereo.py:362-399) for one frame, float32 numpy arrays:
    flow [B,1,H,W] (negative disparity), valid [B,H,W] (the dataset's raw map: 0 / 0.3 / 0.7 / 1, with rectangular holes; all 0
    when `empty`), up [iters,2,B,1,H,W] and q [iters,2,B,1,H/4,W/4] (the [flow, flow_refine] pairs of every iteration), grad
    [iters,B,2,H/4,W/4], flow_mono / flow_init [B,1,H,W], cost_volume [B,W/4,H/4,W/4].
    The disparity is a ramp over the top half (the GT index of init_loss near 0, some below) and near 0 over the bottom half (the
    index near D-1), with a step edge (gradients above the < 5 bound) and a few pixels beyond the |flow| < 700 bound.  The cost
    volume is mostly negative noise with a peak at the GT index, so that the zero fill of masked candidates enters the top-k."""
    gen = np.random.Generator(np.random.Philox(key=int(seed) + 0x10550))
    h, w = H // 4, W // 4
    x = np.arange(W, dtype=np.float64)[None, :]
    disp = np.empty((B, H, W))
    for b in range(B):
        a = gen.uniform(0.85, 1.1)
        top = a * x * np.ones((H // 2, 1)) + gen.normal(0, 0.3, (H // 2, W))
        bot = np.abs(gen.normal(0.15, 0.1, (H - H // 2, W)))
        d = np.concatenate([top, bot], 0)
        c0 = int(gen.integers(W // 4, 3 * W // 4))
        d[:, c0:] += gen.uniform(6, 10)                     # step edge
        d = np.maximum(d, 0.0)
        d[int(gen.integers(0, H)), int(gen.integers(0, W))] = 800.0     # beyond max_flow
        disp[b] = d
    flow = (-disp[:, None]).astype(np.float32)
    valid = gen.choice(np.array([0.0, 0.3, 0.7, 1.0, 1.0, 1.0, 1.0, 1.0]), size=(B, H, W))
    for b in range(B):
        for _ in range(2):
            y0, x0 = int(gen.integers(0, H - 6)), int(gen.integers(0, W - 6))
            valid[b, y0:y0 + int(gen.integers(3, 9)), x0:x0 + int(gen.integers(3, 9))] = 0.0
    valid[:, 4:12, 4:12] = np.where(valid[:, 4:12, 4:12] > 0, 1.0, 0.0)   # a block that survives the bilinear == 1 test
    if empty:
        valid[:] = 0.0
    valid = valid.astype(np.float32)
    up = np.empty((iters, 2, B, 1, H, W), np.float32)
    q = np.empty((iters, 2, B, 1, h, w), np.float32)
    flow_q = flow[:, :, ::4, ::4][:, :, :h, :w] / 4.0
    for i in range(iters):
        s = 6.0 * 0.6 ** i
        up[i] = flow + gen.normal(0, s, up[i].shape) * gen.choice([0.1, 1.0], size=up[i].shape)
        q[i] = flow_q + gen.normal(0, s / 4, q[i].shape)
    grad = gen.normal(0, 0.5, (iters, B, 2, h, w)).astype(np.float32)
    flow_mono = (flow + gen.normal(0, 3.0, flow.shape)).astype(np.float32)
    flow_init = (flow + gen.normal(0, 1.5, flow.shape)).astype(np.float32)
    cv = gen.normal(-0.2, 0.3, (B, w, h, w))
    idx = np.clip(np.arange(w)[None, None, :] + flow_q[:, 0], 0, w - 1)         # [B,h,w]
    peak = np.exp(-0.5 * (np.arange(w)[None, :, None, None] - idx[:, None]) ** 2)
    cv = (cv + 0.9 * peak).astype(np.float32)
    return dict(flow=flow, valid=valid, up=up, q=q.astype(np.float32), grad=grad, flow_mono=flow_mono, flow_init=flow_init,
                cost_volume=cv)


def make_corr_grad_case(seed: int, B: int = 1, C: int = 256, H: int = 3, W: int = 44, radius: int = 4, lookups: int = 3,
                        extreme: bool = True) -> dict:
    """Inputs of one CorrBlock1D training step (corr.py:8-79), float32 numpy arrays: fmap1, fmap2 [B,C,H,W]; coords
    [lookups,B,1,H,W]; g_lookup [lookups,B,4(2r+1),H,W] (upstream gradients of the lookups); g_cost [B,W,H,W] (of the
    cost volume); g_main [B,1,H,W] (of argmax_disp's main_cost).  fmap2 is fmap1 shifted by a per-row disparity plus noise, so
    the volume has a clear winner and argmax_disp's 0.3-margin mask is mostly 1.  Pixel (0, 0, 1) of fmap1 and pixel (0, H-1, 2)
    of fmap2 are all-zero (the F.normalize eps branch).  Coordinates: lookup 0 follows the disparity with fractional offsets,
    lookup 1 is uniform over [-12, W+12] (taps out of range at both ends), lookup 2 is integer-valued; with `extreme`, lookup 2
    also holds +-1000 and +-3e9 at a few pixels."""
    gen = np.random.Generator(np.random.Philox(key=int(seed) + 0xC022))
    T = 2 * radius + 1
    f1 = gen.normal(0, 1, (B, C, H, W))
    f2 = gen.normal(0, 1, (B, C, H, W))
    disp = gen.integers(1, max(2, W // 4), size=(B, H))
    for b in range(B):
        for h in range(H):
            d = int(disp[b, h])
            f2[b, :, h, :W - d] = f1[b, :, h, d:] + gen.normal(0, 0.4, (C, W - d))
    f1[0, :, 0, 1] = 0.0
    f2[0, :, H - 1, 2] = 0.0
    x = np.arange(W, dtype=np.float64)[None, None, :]
    coords = np.empty((lookups, B, 1, H, W))
    for k in range(lookups):
        kind = k % 3
        if kind == 0:
            coords[k, :, 0] = x - disp[:, :, None] + gen.uniform(-1.5, 1.5, (B, H, W))
        elif kind == 1:
            coords[k, :, 0] = gen.uniform(-12, W + 12, (B, H, W))
        else:
            coords[k, :, 0] = np.round(gen.uniform(-6, W + 6, (B, H, W)))
            if extreme:
                flat = coords[k].reshape(-1)
                flat[:4] = [1000.0, -1000.0, 3e9, -3e9]
    g_lookup = gen.normal(0, 1, (lookups, B, 4 * T, H, W))
    g_cost = gen.normal(0, 1, (B, W, H, W))
    g_main = gen.normal(0, 1, (B, 1, H, W))
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)     # noqa: E731
    return dict(fmap1=f32(f1), fmap2=f32(f2), coords=f32(coords), g_lookup=f32(g_lookup), g_cost=f32(g_cost), g_main=f32(g_main))
