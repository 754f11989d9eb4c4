"""CPU-only checks: the C-ABI library loads and exports every symbol include/tcs_mi355.h declares
(no compute calls without a GPU), the drop-in module tree matches the reference's state-dict keys,
the harness maths, loud failure without a device, and the N>1 sharding/gather path on gloo."""
import json
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(**kw):
    from argparse import Namespace
    d = dict(hidden_dims=[128] * 3, shared_backbone=True, corr_levels=4, corr_radius=4, n_downsample=2,
             context_norm="none", slow_fast_gru=False, n_gru_layers=3, mixed_precision=False, init_thres=0.5)
    d.update(kw)
    return Namespace(**d)


def test_library_exports_every_declared_symbol():
    from tcs_mi355 import build, native
    build.build(verbose=False)                      # cross-compiles for gfx950 without a GPU
    header = open(os.path.join(ROOT, "include", "tcs_mi355.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(tcs_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations parsed"
    lib = native.lib()
    for name in declared:
        assert hasattr(lib, name), f"libtcs_mi355.so lacks {name}"
    assert declared == set(native.SIGNATURES), declared ^ set(native.SIGNATURES)
    assert lib.tcs_abi_version() >= 1
    assert lib.tcs_error_string(-1) == b"invalid argument"
    # pure host-side size queries are safe without a GPU
    assert lib.tcs_corr_level_bytes(1, 120, 160, 0) == 120 * 160 * 160 * 4
    assert lib.tcs_corr_level_bytes(1, 120, 160, 3) == 120 * 20 * 160 * 4
    assert lib.tcs_conv_packed_floats(256, 384, 3) == 384 * 9 * 256
    assert lib.tcs_conv_packed_floats(1, 256, 3) == 256 * 9 * 32
    assert lib.tcs_conv_packed_floats(64, 1, 7) == 32 * 49 * 64


def test_conv_desc_layout_matches_header():
    """ctypes mirror of struct tcs_conv_desc: same field order as the header."""
    from tcs_mi355 import native
    header = open(os.path.join(ROOT, "include", "tcs_mi355.h")).read()
    body = header[header.index("typedef struct tcs_conv_desc {"):header.index("} tcs_conv_desc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split("{", 1)[1].split(";"):
        decl = decl.strip()
        if not decl:
            continue
        for part in decl.split(","):
            fields.append(re.sub(r"\[.*?\]", "", part.strip().split()[-1].lstrip("*")))
    assert fields == [f[0] for f in native.ConvDesc._fields_]


def test_conv_s16_desc_layout_matches_header():
    """ctypes mirror of struct tcs_conv_s16_desc: same field order as the header."""
    from tcs_mi355 import native
    header = open(os.path.join(ROOT, "include", "tcs_mi355.h")).read()
    body = header[header.index("typedef struct tcs_conv_s16_desc {"):header.index("} tcs_conv_s16_desc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split("{", 1)[1].split(";"):
        decl = decl.strip()
        if not decl:
            continue
        for part in decl.split(","):
            fields.append(re.sub(r"\[.*?\]", "", part.strip().split()[-1].lstrip("*")))
    assert fields == [f[0] for f in native.ConvS16Desc._fields_]


@pytest.mark.parametrize("tag,kw", [("shared_backbone", {}), ("separate_fnet", dict(shared_backbone=False)),
                                    ("context_norm_batch", dict(context_norm="batch"))])
def test_state_dict_keys_match_reference(key_shapes, tag, kw):
    from core.tc_stereo import TCStereo
    sd = {k: list(v.shape) for k, v in TCStereo(_args(**kw)).state_dict().items()}
    assert sd == key_shapes[tag]


def test_synth_weights_are_deterministic_and_load_strict(key_shapes):
    from core.tc_stereo import TCStereo
    from tcs_mi355.weights import DAMPED_HEADS, synth_state_dict, synth_tensor
    a = synth_state_dict(key_shapes["shared_backbone"])
    b = synth_state_dict(key_shapes["shared_backbone"])
    assert all(torch.equal(a[k], b[k]) for k in a)
    TCStereo(_args()).load_state_dict(a, strict=True)
    k = DAMPED_HEADS[0]
    assert a[k].std().item() < 0.1 * synth_tensor(k.replace("conv2", "conv1"), a[k].shape).std().item() * 2
    assert a["update_block.gru08.convzr.bias"].abs().sum() == 0


def test_no_cpu_fallback_and_inference_only():
    from core.corr import CorrBlock1D
    from core.tc_stereo import TCStereo
    m = TCStereo(_args()).eval()
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(NotImplementedError):
        m(x, x, iters=1, test_mode=False)
    with pytest.raises(RuntimeError, match="no CPU"):
        m(x, x, iters=1, test_mode=True)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        CorrBlock1D(torch.zeros(1, 8, 4, 16), torch.zeros(1, 8, 4, 16))


def test_missing_library_is_loud(monkeypatch, tmp_path):
    from tcs_mi355 import native
    monkeypatch.setattr(native, "_LIB", None)
    monkeypatch.setenv("TCS_MI355_LIB", str(tmp_path / "absent.so"))
    with pytest.raises(native.NativeLibraryMissing):
        native.lib()


def test_input_padder_and_metrics():
    from tcs_mi355.harness import FrameStats, InputPadder, SequenceStats, frame_metrics, reduce_stats
    x = torch.arange(2 * 3 * 375 * 1242, dtype=torch.float32).reshape(2, 3, 375, 1242)
    K = torch.tensor([[[721.5, 0, 609.6], [0, 721.5, 172.9], [0, 0, 1.0]]])
    p = InputPadder(x.shape, divis_by=32)
    (y,), K2 = p.pad(x, K=K)
    assert tuple(y.shape) == (2, 3, 384, 1248)                       # KITTI: 1242x375 -> 1248x384
    assert (p.left, p.right, p.top, p.bottom) == (3, 3, 4, 5)
    assert K2[0, 0, 2].item() == pytest.approx(609.6 + 3) and K2[0, 1, 2].item() == pytest.approx(172.9 + 4)
    assert torch.equal(y[..., 4:379, 3:1245], x)                     # interior untouched
    assert torch.equal(y[..., 0, 3:1245], x[..., 0, :])              # replicate
    z, K3 = p.unpad(y, K=K2)
    assert torch.equal(z, x) and torch.allclose(K3, K)
    # K=None: the bare list, as the reference returns it (core/utils/utils.py:19-28; evaluate_stereo.py:239 unpacks it)
    y1, y2 = p.pad(x, x + 1)
    assert torch.equal(y1, y) and torch.equal(y2, y + 1)
    only = p.pad(x)
    assert isinstance(only, list) and len(only) == 1 and torch.equal(only[0], y)
    q = InputPadder((1, 3, 240, 320), divis_by=32)
    assert (q.top, q.bottom, q.left, q.right) == (8, 8, 0, 0)        # config 1: 240 -> 256 rows
    k = InputPadder((1, 3, 375, 1242), mode="kitti", divis_by=32)
    assert (k.top, k.bottom) == (0, 9)
    gt = torch.tensor([[[[10.0, 200.0], [5.0, 1.0]]]])
    pr = torch.tensor([[[[10.5, 0.0], [9.0, 1.0]]]])
    fs = frame_metrics(pr, gt)                                       # 200 is invalid (>=192)
    assert fs.mask_rate == pytest.approx(0.75)
    assert fs.epe == pytest.approx((0.5 + 4.0 + 0.0) / 3)
    assert fs.d1_weighted == pytest.approx((1 / 3) * 0.75) and fs.d3_weighted == pytest.approx((1 / 3) * 0.75)
    assert frame_metrics(pr, torch.full_like(gt, 500.0)) is None
    s1, s2 = SequenceStats([fs, fs]), SequenceStats([FrameStats(1.0, 0.5, 0.25, 1.0)])
    r = reduce_stats([s1.vector(), s2.vector()])
    assert r["frames"] == 3
    assert r["epe"] == pytest.approx((2 * fs.epe + 1.0) / 3)
    assert r["d1"] == pytest.approx(100 * ((2 * fs.d1_weighted + 0.5) / 3) / ((2 * 0.75 + 1.0) / 3))


def test_synthetic_sequence_properties():
    from tcs_mi355 import synth
    seq = synth.make_sequence(3, n_frames=2, height=96, width=128, max_disp=48.0)
    again = synth.make_sequence(3, n_frames=2, height=96, width=128, max_disp=48.0)
    f = seq.frames[0]
    assert f.image1.shape == (3, 96, 128) and f.image1.dtype == np.float32
    assert np.array_equal(f.image1, again.frames[0].image1)          # deterministic
    assert f.image1.min() >= 0 and f.image1.max() <= 255 and np.array_equal(f.image1, np.rint(f.image1))
    assert 0 < f.disp_gt.min() and f.disp_gt.max() < 48.0
    T0, T1 = seq.frames[0].T, seq.frames[1].T
    assert np.allclose(T0, np.eye(4), atol=1e-6) and not np.allclose(T1, T0)
    assert np.allclose(T1[:3, :3] @ T1[:3, :3].T, np.eye(3), atol=1e-5)
    # stereo consistency: left pixel x matches right pixel x - disp where unoccluded
    d = f.disp_gt[0]
    ys, xs = np.mgrid[0:96, 0:128]
    xr = np.rint(xs - d).astype(int)
    ok = xr >= 0
    err = np.abs(f.image1[:, ys[ok], xs[ok]] - f.image2[:, ys[ok], xr[ok]]).mean()
    assert err < 12.0


def test_two_rank_gloo_shard_and_gather(tmp_path):
    """world_size 2 on gloo: round-robin sequence sharding + the single all_gather of statistics."""
    script = tmp_path / "rank.py"
    script.write_text(textwrap.dedent(f"""
        import sys, json
        sys.path.insert(0, {ROOT!r})
        import tcs_paths; tcs_paths.add_product_path()
        import numpy as np
        from tcs_mi355 import dist as td
        from tcs_mi355.harness import FrameStats, SequenceStats, reduce_stats
        rank, world, local = td.init_from_env(force_backend="gloo")
        mine = td.shard(list(range(5)), rank, world)
        st = SequenceStats([FrameStats(float(s), 0.1 * s, 0.01 * s, 1.0) for s in mine])
        vecs = td.gather_vectors(st.vector())
        slow = td.max_over_ranks(1.0 + rank)
        td.barrier()
        if rank == 0:
            print(json.dumps(dict(mine=mine, n=len(vecs), red=reduce_stats(vecs), slow=slow)))
    """))
    import socket
    with socket.socket() as so:                          # a free port (a fixed one collides with a run that ended seconds ago)
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]
    outs = [p.communicate(timeout=180) for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    res = json.loads(outs[0][0].strip().splitlines()[-1])
    assert res["mine"] == [0, 2, 4] and res["n"] == 2 and res["slow"] == 2.0
    assert res["red"]["frames"] == 5
    assert res["red"]["epe"] == pytest.approx(np.mean([0, 1, 2, 3, 4]))


def test_bench_spawns_its_own_ranks():
    """`python bench.py --gpus 2` outside torchrun starts 2 ranks itself (BASELINE configs[3] is driven this way at N = 8);
    --dry-run swaps the model for a sleep so the launcher, rendezvous, barrier and statistics gather run on CPU over gloo."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--dry-run"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 2 and line["dist_world_size"] == 2 and line["ranks_frames"] == [3, 3] and line["dist_backend"] == "gloo"
    # a torchrun environment whose WORLD_SIZE disagrees with --gpus must fail loudly instead of printing n_gpus: 1
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--dry-run"],
                         env=dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"), capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "WORLD_SIZE" in (bad.stderr + bad.stdout)


def test_tartanair_folder_and_checkpoint_loaders(tmp_path, key_shapes):
    """BASELINE configs[2] plumbing on a constructed 2-frame trajectory folder: file pairing, PNG decoding, depth->disparity,
    pose parsing, and the weights-only checkpoint path with DataParallel-style `module.` keys.  (The readers themselves are
    pinned to the reference's outputs by test_formats_match_reference_fixtures; no dataset or checkpoint exists offline.)"""
    from PIL import Image
    from tcs_mi355 import harness
    from tcs_mi355.weights import synth_state_dict
    root = tmp_path / "abandonedfactory" / "Easy" / "P000"
    for d in ("image_left", "image_right", "depth_left"):
        (root / d).mkdir(parents=True)
    rng = np.random.default_rng(0)
    imgs = rng.integers(0, 256, size=(2, 2, 480, 640, 3), dtype=np.uint8)
    depth = rng.uniform(1.0, 30.0, size=(2, 480, 640)).astype(np.float32)
    for i in range(2):
        Image.fromarray(imgs[i, 0]).save(root / "image_left" / f"{i:06d}_left.png")
        Image.fromarray(imgs[i, 1]).save(root / "image_right" / f"{i:06d}_right.png")
        np.save(root / "depth_left" / f"{i:06d}_left_depth.npy", depth[i])
    (root / "pose_left.txt").write_text("0 0 0 0 0 0 1\n0.1 0.0 0.0 0 0 0 1\n")
    seq = harness.load_tartanair_sequence(str(root))
    assert seq is not None and len(seq.frames) == 2 and seq.baseline == 0.25
    f1 = seq.frames[1]
    assert f1.image1.shape == (3, 480, 640) and f1.image1.dtype == np.float32
    assert np.array_equal(f1.image1, imgs[1, 0].transpose(2, 0, 1).astype(np.float32))
    assert np.array_equal(f1.image2, imgs[1, 1].transpose(2, 0, 1).astype(np.float32))
    assert np.allclose(f1.disp_gt[0], 80.0 / (depth[1] + 1e-5))
    # camera 0.1 m along NED x (forward) -> world->camera translation -0.1 along camera z
    assert np.allclose(f1.T[:3, 3], [0, 0, -0.1], atol=1e-6) and np.allclose(seq.frames[0].T, np.eye(4)[[1, 2, 0, 3]] @ np.eye(4), atol=1e-6)
    assert harness.load_tartanair_sequence(str(tmp_path / "nope")) is None and "not a directory" in harness.load_tartanair_sequence.why
    (root / "pose_left.txt").unlink()
    assert harness.load_tartanair_sequence(str(root)) is None and "pose_left.txt missing" in harness.load_tartanair_sequence.why
    # checkpoint: {'model': state_dict with 'module.' prefixes}
    from core.tc_stereo import TCStereo
    W = synth_state_dict(key_shapes["shared_backbone"])
    torch.save({"model": {"module." + k: v for k, v in W.items()}, "optimizer": {}}, tmp_path / "tc.pth")
    m = TCStereo(_args())
    assert harness.load_checkpoint(m, str(tmp_path / "tc.pth")) == len(W)
    k0 = "update_block.gru08.convq.weight"
    assert torch.equal(m.state_dict()[k0], W[k0])
    bad = dict(W)
    bad.pop(k0)
    torch.save({"model": bad}, tmp_path / "bad.pth")
    with pytest.raises(RuntimeError):
        harness.load_checkpoint(TCStereo(_args()), str(tmp_path / "bad.pth"))


def test_formats_known_answers(tmp_path):
    """N2 file formats: known-answer checks against scipy's Rotation — the function the reference itself calls
    (frame_utils.py:244) — and round trips.  The reference-generated vectors are in test_formats_match_reference_fixtures."""
    from scipy.spatial.transform import Rotation
    from tcs_mi355 import formats
    rng = np.random.default_rng(0)
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    t = rng.normal(size=3)
    assert np.allclose(formats.quat_to_matrix(*q), Rotation.from_quat(q).as_matrix(), atol=1e-12)
    # frame_utils.py:245-257 restated with scipy
    R = Rotation.from_quat(q).as_matrix()
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R.T, -R.T @ t
    m = np.zeros((4, 4))
    m[0, 1] = m[1, 2] = m[2, 0] = m[3, 3] = 1
    want = m @ T
    p = tmp_path / "pose_left.txt"
    p.write_text(" ".join(f"{v:.12f}" for v in (*t, *q)) + "\n" + "0 0 0 0 0 0 1\n")
    got = formats.read_tartanair_extrinsic(str(p))
    assert len(got) == 2 and np.allclose(got[0], want, atol=1e-9)
    assert np.allclose(got[1], m)                                     # identity pose -> pure axis permutation
    # KITTI: 3x4 camera->world rows, inverted
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = R, t
    k = tmp_path / "kitti.txt"
    k.write_text(" ".join(f"{v:.12f}" for v in P[:3].ravel()) + "\n")
    assert np.allclose(formats.read_kitti_extrinsic(str(k))[0] @ P, np.eye(4), atol=1e-9)
    s = tmp_path / "camera_data.txt"
    s.write_text("Frame 1\nL " + " ".join(f"{v:.12f}" for v in P.ravel()) + "\nR " + " ".join(["0"] * 16) + "\n\n")
    sf = formats.read_sceneflow_pose(str(s))
    assert len(sf) == 1 and np.allclose(sf[0] @ P, np.eye(4), atol=1e-9)
    # TartanAir depth -> disparity
    d, v = formats.disp_from_tartanair_depth(np.array([[1.0, 80.0], [0.0, 1e9]]))
    assert d[0, 0] == pytest.approx(80.0 / 1.00001) and d[0, 1] == pytest.approx(1.0, rel=1e-6) and v.all()
    # PFM round trip (bottom-up rows, little endian) + a hand-built big-endian file
    img = rng.normal(size=(5, 7)).astype(np.float32)
    f = tmp_path / "d.pfm"
    formats.write_pfm(str(f), img)
    assert np.array_equal(formats.read_pfm(str(f)), img)
    be = tmp_path / "be.pfm"
    be.write_bytes(b"Pf\n2 2\n1.0\n" + np.array([[3, 4], [1, 2]], ">f4").tobytes())
    assert np.array_equal(formats.read_pfm(str(be)), np.array([[1, 2], [3, 4]], np.float32))


def test_formats_match_reference_fixtures(tmp_path):
    """N2 pinned to the reference: tests/golden/formats.npz holds constructed input files (as bytes) and what the REFERENCE's
    readers (core/utils/frame_utils.py, imported by tools/make_goldens_formats.py with stub cv2 / imageio modules) returned for
    them.  tcs_mi355/formats.py and the harness' PNG reader must reproduce those outputs: poses to 1e-12 (same float64
    algebra, scipy vs a closed-form quaternion matrix), everything else exactly."""
    from tcs_mi355 import formats, harness
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "formats.npz")))

    def put(name, key):
        p = tmp_path / name
        p.write_bytes(g[key].tobytes())
        return str(p)

    got = np.stack(formats.read_tartanair_extrinsic(put("pose_left.txt", "tartanair_pose_txt")))
    assert got.shape == g["tartanair_pose_out"].shape and np.abs(got - g["tartanair_pose_out"]).max() <= 1e-12
    disp, valid = formats.read_disp_tartanair(put("000000_left_depth.npy", "tartanair_depth_npy"))
    assert disp.dtype == g["tartanair_disp_out"].dtype and np.array_equal(disp, g["tartanair_disp_out"])
    assert np.array_equal(valid, g["tartanair_valid_out"])
    for name in ("pfm_le", "pfm_be", "pfm_color"):
        a = formats.read_pfm(put(name + ".pfm", name + "_file"))
        assert a.shape == g[name + "_out"].shape and np.array_equal(a, g[name + "_out"]), name
        b = formats.read_gen_pfm(str(tmp_path / (name + ".pfm")))
        assert b.shape == g[name + "_gen_out"].shape and np.array_equal(b, g[name + "_gen_out"]), name
    got = np.stack(formats.read_kitti_extrinsic(put("poses.txt", "kitti_pose_txt")))
    assert np.abs(got - g["kitti_pose_out"]).max() <= 1e-12
    got = np.stack(formats.read_sceneflow_pose(put("camera_data.txt", "sceneflow_pose_txt")))
    assert got.shape == g["sceneflow_pose_out"].shape and np.abs(got - g["sceneflow_pose_out"]).max() <= 1e-12
    img = harness._read_rgb(put("000000_left.png", "png_file"))
    assert img.dtype == np.float32 and np.array_equal(img, g["png_out"])


def test_bench_dump_outputs(tmp_path):
    """bench.py --dump-outputs: every array of the forward() dict as float32 <name>.npy; above the size limit, the same seeded
    sample of each array on every run, and the files together stay under the limit.  --steps below 1 is refused."""
    sys.path.insert(0, ROOT)
    import bench
    gen = torch.Generator().manual_seed(3)
    out = {"flow": torch.randn(2, 1, 64, 96, generator=gen), "flow_q": torch.randn(2, 1, 16, 24, generator=gen),
           "fmap1": torch.randn(2, 256, 16, 24, generator=gen).double(),
           "net_list": [torch.randn(2, 128, 16, 24, generator=gen), torch.randn(2, 128, 8, 12, generator=gen), torch.randn(2, 128, 4, 6, generator=gen)]}
    names = ["flow", "flow_q", "fmap1", "net_list_0", "net_list_1", "net_list_2"]
    full = bench.dump_outputs(str(tmp_path / "full"), out)
    assert not full["sampled"] and sorted(full["arrays"]) == sorted(names)
    for n in names:
        a = np.load(tmp_path / "full" / f"{n}.npy")
        want = out[n] if n in out else out["net_list"][int(n[-1])]
        assert a.dtype == np.float32 and a.shape == tuple(want.shape) and np.array_equal(a, want.float().numpy()), n
    limit = 200_000
    runs = [bench.dump_outputs(str(tmp_path / d), out, limit=limit) for d in ("s1", "s2")]
    assert runs[0]["sampled"] and runs[0] == dict(runs[1], dir=runs[0]["dir"])
    assert sum(os.path.getsize(tmp_path / "s1" / f"{n}.npy") for n in names) <= limit
    for n in names:
        a, b = np.load(tmp_path / "s1" / f"{n}.npy"), np.load(tmp_path / "s2" / f"{n}.npy")
        assert a.dtype == np.float32 and a.ndim == 1 and a.size == runs[0]["arrays"][n]["sample"] and np.array_equal(a, b), n
        assert np.isin(a, np.load(tmp_path / "full" / f"{n}.npy")).all(), n
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0", "--dry-run"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--steps" in r.stderr


def test_gpu_count_from_kfd_topology(tmp_path, monkeypatch):
    """bench.py's launcher counts GPUs from the KFD topology in sysfs (no HIP / amdsmi call in the parent of the ranks)."""
    sys.path.insert(0, ROOT)
    import bench
    for i, simd in enumerate((0, 0, 256, 256, 256)):                   # two CPU nodes, three GPUs
        d = tmp_path / str(i)
        d.mkdir()
        (d / "properties").write_text(f"cpu_cores_count {16 if simd == 0 else 0}\nsimd_count {simd}\nmem_banks_count 1\n")
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        monkeypatch.delenv(var, raising=False)
    assert bench.count_gpus_sysfs(str(tmp_path)) == 3
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "0,2")
    assert bench.count_gpus_sysfs(str(tmp_path)) == 2
    assert bench.count_gpus_sysfs(str(tmp_path / "missing")) is None


def test_kernel_register_budgets():
    """The occupancy of the loop's convolution kernel is decided by its register allocation, and the allocation by its epilogue, not by
    its K loop: round 3 shipped, for a day, LINEAR instances at 220 VGPRs (two waves per SIMD) without any test
    noticing.  Read the built library's code-object metadata (tools/kernel_resources.py; no GPU) and hold the instances the frame uses
    to their budgets; no kernel of the library may spill."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    if not os.path.exists(f"{kr.LLVM}/clang-offload-bundler") or not os.path.exists(f"{kr.LLVM}/llvm-readelf"):
        pytest.skip("LLVM binary utilities not found")
    from tcs_mi355 import native
    res = kr.kernel_resources(native.lib_path())
    assert len(res) > 150, len(res)
    names = sorted(res)
    nice = dict(zip(names, kr.demangle(names)))
    spilled = [nice[k] for k in names if res[k].get("vgpr_spill_count", 0)]          # (SGPRs spilled to VGPR lanes cost no memory traffic)
    assert not spilled, spilled
    seen = {"linear": 0, "gru_zr": 0, "gru_q": 0, "taps": 0}
    for k in names:
        m = re.match(r"void k_conv_s16<(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (true|false)>", nice[k])
        if not m:
            continue
        ks, mt, rows, kst, nst, stride, epi, rs, rpw = (int(v) for v in m.groups()[:9])
        tp = m.group(10) == "true"
        v = res[k]["vgpr_count"]
        if mt != 1 or rpw != 1:
            continue                                    # 64-channel and two-row tiles: options the heuristic does not pick
        if tp:
            assert v <= 128, (nice[k], v)               # four waves per SIMD
            seen["taps"] += 1
        elif epi == 0:
            assert v <= 96, (nice[k], v)                # five
            seen["linear"] += 1
        elif epi == 1:
            assert v <= 104, (nice[k], v)               # four (96 would cost spills: s16_min_waves)
            seen["gru_zr"] += 1
        elif epi == 2:
            assert v <= 128, (nice[k], v)
            seen["gru_q"] += 1
    assert all(n > 0 for n in seen.values()), seen
    # grouped launches (two tile instances behind a branch on the block index): the allocation is the larger of the two bodies' and must
    # stay at the LINEAR budget, or both halves of a pair lose a wave per SIMD
    pairs = [k for k in names if nice[k].startswith("void k_conv_s16_pair<")]
    assert len(pairs) >= 3, [nice[k] for k in pairs]
    for k in pairs:
        assert res[k]["vgpr_count"] <= 96, (nice[k], res[k]["vgpr_count"])


def test_forking_is_switched_off_below_three_hardware_queues():
    """tcs_mi355/streams.py: with GPU_MAX_HW_QUEUES < 3 the captured frame's parallel launch lists deadlock on ROCm 7.2 (rounds 2-3: no frame
    completes); the module then runs every frame as one launch list.  Checked in a child interpreter per setting (the switch is read at import)."""
    import subprocess
    import sys
    code = ("import sys, warnings; sys.path.insert(0, %r); import tcs_paths; tcs_paths.add_product_path(); warnings.simplefilter('ignore'); "
            "from tcs_mi355 import streams; print(int(streams.ENABLED))" % ROOT)
    for val, want in (("", "1"), ("3", "1"), ("2", "0")):
        env = dict(os.environ)
        env.pop("TCS_MI355_STREAMS", None)
        if val:
            env["GPU_MAX_HW_QUEUES"] = val
        else:
            env.pop("GPU_MAX_HW_QUEUES", None)
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-500:]
        assert out.stdout.strip().splitlines()[-1] == want, (val, out.stdout)


def test_lookup_profile_rows_are_selected_by_grid_size(tmp_path):
    """tools/make_lookup_pmc_json.py on the committed round-3 folds: the four-sequence row must be the BATCHED kernel's (k_corr_lookup<4, 4>,
    9.25 us in loop position = 0.32 of the roofline), not the one-sequence launches of the same trace's evaluation pass (5.48 us — which round 3
    divided into four sequences' bytes and reported as 0.54)."""
    import json
    import subprocess
    import sys
    out = tmp_path / "lk.json"
    prof = os.path.join(ROOT, "profiles")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_lookup_pmc_json.py"),
                    "--row", f"one_sequence_640x480:{prof}/r03_bench_kernel_trace_fold.csv:19200",
                    "--row", f"four_sequences_640x480:{prof}/r03_bench_4seq_kernel_trace_fold.csv:76800",
                    "--row", f"kitti_375x1242:{prof}/r03_bench_kitti_kernel_trace_fold.csv:29952", "--out", str(out)],
                   check=True, capture_output=True, timeout=120)
    d = json.load(open(out))["workloads"]
    four = d["four_sequences_640x480"]
    assert "<4, 4>" in four["rocprof_loop_kernel"] and abs(four["rocprof_loop_avg_us"] - 9.254) < 1e-3
    assert abs(four["frac_rocprof_loop"] - 0.3195) < 2e-3 and abs(four["frac_rocprof_burst"] - 0.4934) < 2e-3
    assert "<4, 1>" in d["one_sequence_640x480"]["rocprof_loop_kernel"] and "<4, 1>" in d["kitti_375x1242"]["rocprof_loop_kernel"]


@pytest.mark.skipif(torch.cuda.is_available(), reason="descriptors with fake device pointers: host-only check")
def test_conv_group_fused_query_answers_on_the_host():
    """The answers of tcs_conv2d_group_fused, computed on the host: the fp32-MFMA pair of DispGradPredictor's stems at 120x160 is one
    launch; at batch 4 (32 -> 64 takes the 64-wide tile), with mismatched batches, or with a layer that has no planned kernel
    (fp16-split, Cin == 1) it is two.  (This checks the answers only; that the query makes no launch is a property of the code in
    tcs_conv2d, where every launch without a planner is preceded by conv_query_only().)  The descriptors carry fake device pointers,
    so the test runs only where no GPU is visible."""
    import ctypes as C

    from tcs_mi355 import native
    lib = native.lib()
    fake = 0x10000                                      # never dereferenced: nothing is launched

    def desc(cin, cout, B, H=120, W=160, math=0):
        d = native.ConvDesc()
        d.src[0], d.src_ch[0], d.n_src = fake, cin, 1
        d.weight, d.out = fake, fake
        d.B, d.H, d.W, d.Cin, d.Cout, d.ksize = B, H, W, cin, cout, 3
        d.post_scale, d.out_ctot, d.math, d.weight_unscale = 1.0, cout, math, 1.0
        return d

    def fused(a, b):
        arr = (C.POINTER(native.ConvDesc) * 2)(C.pointer(a), C.pointer(b))
        return lib.tcs_conv2d_group_fused(arr, 2)

    assert fused(desc(2, 32, 1), desc(32, 64, 1)) == 1
    assert fused(desc(2, 32, 1, 61, 83), desc(32, 64, 1, 61, 83)) == 1
    assert fused(desc(2, 32, 4), desc(32, 64, 4)) == 0
    assert fused(desc(2, 32, 2), desc(32, 64, 1)) == 0
    assert fused(desc(32, 32, 1, math=1), desc(2, 32, 1)) == 0
    assert fused(desc(2, 32, 1), desc(32, 32, 1, math=1)) == 0
    assert fused(desc(1, 32, 1), desc(2, 32, 1)) == 0
    assert fused(desc(2, 32, 1), desc(2, 32, 1, 0, 160)) == 0      # invalid descriptor
    arr = (C.POINTER(native.ConvDesc) * 1)(C.pointer(desc(2, 32, 1)))
    assert lib.tcs_conv2d_group_fused(arr, 1) == 0
