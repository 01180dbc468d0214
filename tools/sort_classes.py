"""Which run sizes the sort stage of the bench workload meets: the short lists by ceil(n / 64) (one wave, n <= 512) and ceil(n / 256)
(four waves, 513 .. 2048), the parts of the part list by ceil(c / 64) -- the keys per lane fr_sortnet.h's dispatch gives them -- with
the share of positions that are padding under that dispatch and under the power-of-two dispatch (1, 2, 4, 8 / 4, 8) it replaced."""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "fisher-nerf-customized_amd"))
import numpy as np, torch
from fisher_rast import synthetic, _lib
from fisher_rast.ops import FisherScorer
from models.SLAM.utils.recon_helpers import setup_camera
dev = torch.device("cuda:0")
P, V, W, H = 500_000, 64, 256, 256
act = synthetic.activate(synthetic.room_shell(P, 2))
cam = setup_camera(W, H, synthetic.intrinsics(W, H), np.eye(4), device=dev)
sc = FisherScorer(cam, *(act[k].to(dev) for k in ("means3D", "rgb_colors", "rotations", "opacities", "scales")))
w2c = synthetic.invert_rigid(synthetic.candidate_poses(V, 2)).to(dev)
sc.run(w2c, H_inv=torch.rand((P, 4), device=dev))
torch.cuda.synchronize()
lib = _lib.load()
cap = V * sc._keys_per_view()
off = (ctypes.c_size_t * 8)()
_lib.check(lib.fr_fisher_workspace_layout(P, W, H, V, cap, 4, off), "layout")
po = ctypes.c_size_t(0)
_lib.check(lib.fr_fisher_part_list_offset(P, W, H, V, cap, 4, ctypes.byref(po)), "part list offset")
ws = sc._ws[0]
T = (W // 16) * (H // 16)
cnt = ws[off[0]:off[0] + V * T * 4].view(torch.int32).cpu().numpy().astype(np.int64)
n_parts = int(ws[po.value:po.value + 4].view(torch.int32).cpu().numpy()[0])
parts = ws[po.value + 64:po.value + 64 + n_parts * 8].view(torch.int32).cpu().numpy().astype(np.int64).reshape(-1, 2)[:, 1]


def table(name, n, per):
    """n: run lengths; per: keys per unit of K (64: one wave, 256: four waves)"""
    k_new = (n + per - 1) // per
    k_old = np.where(k_new <= 1, 1, np.where(k_new <= 2, 2, np.where(k_new <= 4, 4, 8))) if per == 64 else np.where(k_new <= 4, 4, 8)
    print(f"{name}: {n.size} runs, {n.sum()} keys, mean {n.mean():.0f}; positions sorted {int((k_new * per).sum())} (padding {1 - n.sum() / (k_new * per).sum():.1%})"
          f" against {int((k_old * per).sum())} (padding {1 - n.sum() / (k_old * per).sum():.1%}) with K a power of two")
    for K in range(1, 9):
        m = k_new == K
        if m.any():
            print(f"  K = {K}: {int(m.sum()):6d} runs  {int(n[m].sum()):9d} keys  mean {n[m].mean():6.0f}")


table("short lists, one wave (2 .. 512)", cnt[(cnt >= 2) & (cnt <= 512)], 64)
table("short lists, four waves (513 .. 2048)", cnt[(cnt >= 513) & (cnt <= 2048)], 256)
table("parts (2 .. 512)", parts, 64)
