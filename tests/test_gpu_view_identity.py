"""-m gpu: the identity-view front end (fr_fisher_cfg.view_is_identity, k_preprocess_views_c<4, 0, true, true>).
  * the identity path and the general one (the hint cleared, same identity camera) give the same counts exactly, scores within 1e-5;
  * a camera whose view matrix is not the identity (no hint) still matches the oracle;
  * a wrong hint is reported, and nothing is scored;
  * bench.py's 10k-Gaussian, 8-view workload (BASELINE configs[0]) reproduces the outputs the general build recorded
    (tests/golden/bench_10k_v8_outputs.npz): counts exactly, scores within 1e-5."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("means3D", "rgb_colors", "rotations", "opacities", "scales")


def _scene(P, V, W, H, seed, cam_w2c=None, dev="cuda:0"):
    from fisher_rast import synthetic
    from models.SLAM.utils.recon_helpers import setup_camera
    act = synthetic.activate(synthetic.room_shell(P, seed=seed))
    w2c = synthetic.invert_rigid(synthetic.candidate_poses(V, seed=seed + 10))
    K = synthetic.intrinsics(W, H)
    view = np.eye(4) if cam_w2c is None else cam_w2c
    cam = setup_camera(W, H, K, view, device=torch.device(dev))
    return act, w2c, K, cam


def _scorer(cam, act, dev):
    from fisher_rast.ops import FisherScorer
    return FisherScorer(cam, *(act[k].to(dev) for k in KEYS))


def test_identity_and_general_paths_agree(gpu):
    P, V, W, H = 60000, 16, 256, 256
    act, w2c, _, cam = _scene(P, V, W, H, seed=3)
    a, b = _scorer(cam, act, gpu), _scorer(cam, act, gpu)
    assert a.view_is_identity
    b.view_is_identity = False
    Hi = torch.rand((P, 4), generator=torch.Generator().manual_seed(5)).to(gpu) + 0.05
    ra = a.run(w2c.to(gpu), H_inv=Hi)
    rb = b.run(w2c.to(gpu), H_inv=Hi)
    torch.cuda.synchronize()
    assert np.array_equal(ra["vis_count"].cpu().numpy(), rb["vis_count"].cpu().numpy())
    assert np.array_equal(ra["num_rendered"].cpu().numpy(), rb["num_rendered"].cpu().numpy())
    assert (ra["vis_count"].cpu().numpy() > 0).all()
    sa, sb = ra["scores"].cpu().double().numpy(), rb["scores"].cpu().double().numpy()
    assert np.isfinite(sa).all() and (sa > 0).all()
    assert np.abs(sa - sb).max() / np.abs(sb).max() <= 1e-5, (sa, sb)
    assert (np.abs(sa - sb) <= 1e-5 * np.abs(sb)).all(), (sa, sb)


def test_non_identity_camera_matches_oracle(gpu):
    from fisher_rast import synthetic
    from oracle import ref
    P, V, W, H = 4000, 4, 128, 128
    c, s = np.cos(0.08), np.sin(0.08)
    cam_w2c = np.array([[c, 0, s, 0.05], [0, 1, 0, -0.03], [-s, 0, c, 0.02], [0, 0, 0, 1]], np.float32)
    act, w2c, K, cam = _scene(P, V, W, H, seed=1, cam_w2c=cam_w2c)
    sc = _scorer(cam, act, gpu)
    assert not sc.view_is_identity
    rng = np.random.default_rng(2)
    H_train = rng.uniform(0.0, 2.0, (P, 4)).astype(np.float32)
    got = sc.run(w2c.to(gpu), H_inv=torch.reciprocal(torch.from_numpy(H_train).to(gpu) + 0.1))
    torch.cuda.synchronize()
    ocam = ref.setup_camera(W, H, K, cam_w2c)
    args = tuple(act[k].numpy() for k in KEYS)
    want, vis = ref.pose_eval(ocam, w2c.numpy(), H_train, *args)
    assert np.array_equal(got["vis_count"].cpu().numpy(), vis)
    s_ = got["scores"].cpu().double().numpy()
    assert np.abs(s_ - want).max() / np.abs(want).max() < 1e-4, (s_, want)


def test_wrong_hint_is_reported(gpu):
    from fisher_rast._lib import FisherRastError
    P, V, W, H = 20000, 8, 256, 256
    cam_w2c = np.eye(4, dtype=np.float32)
    cam_w2c[0, 3] = 0.01
    act, w2c, _, cam = _scene(P, V, W, H, seed=4, cam_w2c=cam_w2c)
    sc = _scorer(cam, act, gpu)
    assert not sc.view_is_identity
    sc.view_is_identity = True
    Hi = torch.ones((P, 4), device=gpu)
    with pytest.raises(FisherRastError, match="view_is_identity"):
        sc.run(w2c.to(gpu), H_inv=Hi)
    r = sc.launch(w2c.to(gpu), H_inv=Hi)
    st = r["status"].cpu().numpy()
    assert st[1] == 1 and st[3] & 2, st                # the overflow flag: nothing scored
    sc.view_is_identity = False                         # the same scorer on the general path
    r = sc.run(w2c.to(gpu), H_inv=Hi)
    assert np.isfinite(r["scores"].cpu().numpy()).all()


def test_bench_10k_8_views_reproduces_recorded_outputs(gpu, tmp_path):
    want = np.load(os.path.join(ROOT, "tests", "golden", "bench_10k_v8_outputs.npz"))
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--gaussians", "10000", "--views", "8", "--steps", "1", "--warmup", "0",
                        "--cpu-views", "0", "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    got = {k: np.load(out / f"{k}.npy") for k in ("scores", "vis_count", "num_rendered")}
    assert np.array_equal(got["vis_count"], want["vis_count"])
    assert np.array_equal(got["num_rendered"], want["num_rendered"])
    s, w = got["scores"].astype(np.float64), want["scores"].astype(np.float64)
    assert (np.abs(s - w) <= 1e-5 * np.abs(w)).all(), (s, w)
