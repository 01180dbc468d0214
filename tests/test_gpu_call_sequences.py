"""-m gpu: a FisherScorer is a long-lived object that a planner calls hundreds of times in every mode; it keeps state between the
calls (workspace, fr_fisher_cfg.reuse_static, the tile-segment sizes).  A seeded random sequence of calls on ONE scorer must give, call
by call, what a FRESH scorer gives for the same call: scores bit for bit (they are deterministic), diagonals to the order of their
float atomics.  Now and then the map itself changes in place between two calls (the scorer holds the caller's tensors); the fresh
scorer of that step is built on the changed map."""
import numpy as np
import pytest
import torch

from scenes import rel_err

pytestmark = pytest.mark.gpu


def _update_map(act, name, rng):
    """an in-place step on a random half of the Gaussians that keeps the map valid (unit quaternions, colours and opacities in [0, 1])"""
    t = act[name]
    sel = torch.from_numpy(rng.random(t.shape[0]) < 0.5).to(t.device)
    step = torch.from_numpy(rng.standard_normal(tuple(t.shape)).astype(np.float32)).to(t.device)
    with torch.no_grad():
        if name == "means3D":
            t[sel] += 0.05 * step[sel]
        elif name == "rgb_colors":
            t[sel] = (t[sel] + 0.2 * step[sel]).clamp(0, 1)
        elif name == "rotations":
            t[sel] = torch.nn.functional.normalize(t[sel] + 0.3 * step[sel])
        elif name == "opacities":
            t[sel] = (t[sel] * torch.exp(0.3 * step[sel])).clamp(0.01, 0.99)
        else:
            t[sel] *= torch.exp(0.2 * step[sel])


@pytest.mark.parametrize("columns,seed", [(4, 0), (4, 1), (11, 2)])
def test_random_call_sequences_equal_fresh_scorers(gpu, columns, seed):
    from fisher_rast import synthetic
    from fisher_rast.ops import FisherScorer
    from models.SLAM.utils.recon_helpers import setup_camera
    P, W, H, NV = 12000, 112, 80, 24
    act = {k: v.to(gpu) for k, v in synthetic.activate(synthetic.room_shell(P, seed=50 + seed)).items()}
    cam = setup_camera(W, H, synthetic.intrinsics(W, H), np.eye(4), device=gpu)
    w2c_all = synthetic.invert_rigid(synthetic.candidate_poses(NV, seed=60 + seed)).to(gpu)
    args = [act[k] for k in ("means3D", "rgb_colors", "rotations", "opacities", "scales")]
    sc = FisherScorer(cam, *args, columns=columns)
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(seed)
    shared = [(torch.rand((P, columns), generator=g) * 2 + 0.05).to(gpu) for _ in range(2)]
    modes = ["score", "score", "score_same", "score_per_view", "outh", "outh_per_view", "both", "image"]
    last_shared = shared[0]
    upd = np.random.default_rng(100 + seed)                          # (its own stream: the sequence of calls stays what it was)
    n_updates = 0
    for step in range(28):
        mode = modes[int(rng.integers(len(modes)))]
        V = int(rng.choice([1, 2, 3, 8, 9, 16]))
        v0 = int(rng.integers(0, NV - V + 1))
        w = w2c_all[v0:v0 + V]
        if upd.random() < 0.25:
            # the map changes in place between two calls (an optimiser step on one of the tensors the scorer holds)
            n_updates += 1
            _update_map(act, str(upd.choice(["means3D", "rgb_colors", "rotations", "opacities", "scales"])), upd)
        fresh = FisherScorer(cam, *args, columns=columns)
        kw = {}
        if mode == "score":
            last_shared = shared[int(rng.integers(2))]
            if rng.random() < 0.3:
                last_shared.mul_(1.5)                                   # in place: same tensor, new version
            kw = dict(H_inv=last_shared)
        elif mode == "score_same":
            kw = dict(H_inv=last_shared)
        elif mode == "score_per_view":
            kw = dict(H_inv=(torch.rand((V, P, columns), generator=g) + 0.05).to(gpu), H_inv_per_view=True)
        elif mode == "image":
            kw = dict(dL_image=(torch.randn((V, 3, H, W), generator=g) * 1e-3).to(gpu))
        elif mode == "both":
            kw = dict(H_inv=(torch.rand((V, P, columns), generator=g) + 0.05).to(gpu), H_inv_per_view=True)
        outs = []
        for s in (sc, fresh):
            k2 = dict(kw)
            if mode in ("outh", "image"):
                k2["out_H"] = torch.zeros((P, columns), device=gpu)
            elif mode in ("outh_per_view", "both"):
                k2["out_H"] = torch.zeros((V, P, columns), device=gpu)
                k2["out_H_per_view"] = True
            r = s.run(w, **k2)
            outs.append((r, k2.get("out_H")))
        (ra, Ha), (rb, Hb) = outs
        assert torch.equal(ra["vis_count"], rb["vis_count"]) and torch.equal(ra["num_rendered"], rb["num_rendered"]), (step, mode)
        if ra["scores"] is not None:
            if mode == "both":            # (the two-pass kernel sums its scores with atomics)
                assert rel_err(ra["scores"].cpu().numpy(), rb["scores"].cpu().numpy()) < 1e-5, (step, mode, V)
            else:
                assert torch.equal(ra["scores"], rb["scores"]), (step, mode, V, ra["scores"], rb["scores"])
            assert float(ra["scores"].min()) > 0
        if Ha is not None:
            assert float(Hb.abs().max()) > 0 and rel_err(Ha.cpu().numpy(), Hb.cpu().numpy()) < 1e-5, (step, mode, V)
    assert n_updates > 0
