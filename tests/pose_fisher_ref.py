"""Test-side reference of the camera-pose Fisher information (fr_fisher_pose_views, include/fisher_rast.h), built from the oracle.

Per pixel p: a one-hot upstream-gradient image (dL on the three channels of p, zero elsewhere) through the oracle's
rasterize_backward(power=1) gives dL_dmeans3D = g_{p,i} for every Gaussian i (the mean2D path and the cov2D-through-J(t) path,
oracle/fisher_oracle.c, cur_dL_dmeans); then j_p = sum_i [g_{p,i}; m_i x g_{p,i}] and pose_H = sum_p j_p j_p^T.
Pixels whose contributor lists share no Gaussian go through one backward call together (the backward is linear in the image and a
Gaussian's gradient then comes from one pixel of the group only), which keeps a view of small splats at tens of calls instead of one per pixel.
The backward runs in the arbiter build (binary64 on the binary32 run's decisions, oracle/ref.py)."""
import numpy as np

from oracle import ref


def _groups(fwd, W, H):
    """pixels with contributors, greedily grouped so that no two pixels of a group share a Gaussian of their lists' prefixes"""
    gx = (W + 15) // 16
    ranges, pl, nc = fwd["ranges"], fwd["point_list"], fwd["n_contrib"]
    P = fwd["radii"].shape[0]
    groups = []
    for py in range(H):
        for px in range(W):
            n = int(nc[py, px])
            if n == 0:
                continue
            t = (py // 16) * gx + px // 16
            ids = np.asarray(pl[int(ranges[t, 0]):int(ranges[t, 0]) + n], dtype=np.int64)
            for used, pix in groups:
                if not used[ids].any():
                    used[ids] = True
                    pix.append((py, px, ids))
                    break
            else:
                used = np.zeros(P, dtype=bool)
                used[ids] = True
                groups.append((used, [(py, px, ids)]))
    return groups


def arbiter_forward(cam, w2c, sc):
    """(binary32 oracle forward, arbiter forward on its decisions, camera-frame means in binary64) of the view w2c"""
    pts = ref.transform_points(w2c, sc["means3D"])
    kw = dict(colors_precomp=sc["colors"], scales=sc["scales"], rotations=sc["rotations"])
    f32 = ref.rasterize_forward(cam, pts, sc["opacities"], **kw)
    m64 = ref.transform_points(w2c, sc["means3D"], arbiter=True)
    f64 = ref.rasterize_forward(cam, m64, sc["opacities"], decisions=f32, **kw)
    return f32, f64, m64


def _run_groups(cam, w2c, sc, dL, groups):
    """j_p and J+_p of the pixels of `groups` (lists of (py, px, ids)): one backward call per group"""
    W, H = cam.image_width, cam.image_height
    _, f64, m64 = arbiter_forward(cam, w2c, sc)
    out = []
    for pix in groups:
        img = np.zeros((3, H, W), dtype=np.float32)
        for py, px, _ in pix:
            img[:, py, px] = np.float32(dL)
        g = ref.rasterize_backward(cam, f64, img, power=1)["dL_dmeans3D"]
        for py, px, ids in pix:
            gi = g[ids]
            e = np.concatenate([gi, np.cross(m64[ids], gi)], axis=1)
            out.append((py, px, e.sum(axis=0), np.abs(e).sum(axis=0)))
    return out


def pose_hessian_ref(cam, w2c, sc, dL=1e-3):
    """Returns (H64 [6,6], JJ [6,6], j [H,W,6]): the arbiter's pose Fisher matrix, sum_p J+_p J+_p^T with
    J+_p = sum_i |[g_{p,i}; m_i x g_{p,i}]| (elementwise: the size of the terms a pixel's sum is made of), and the per-pixel j_p."""
    W, H = cam.image_width, cam.image_height
    f32, _, _ = arbiter_forward(cam, w2c, sc)
    jp = np.zeros((H, W, 6))
    ja = np.zeros((H, W, 6))
    for py, px, j, a in _run_groups(cam, w2c, sc, dL, [pix for _, pix in _groups(f32, W, H)]):
        jp[py, px] = j
        ja[py, px] = a
    j2 = jp.reshape(-1, 6)
    a2 = ja.reshape(-1, 6)
    return j2.T @ j2, a2.T @ a2, jp


def k_needed(got, H64, JJ, rel=1e-4):
    """smallest k with |got - H64| <= rel |H64| + k 2^-24 JJ on every entry"""
    excess = np.abs(np.asarray(got, np.float64) - H64) - rel * np.abs(H64)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(excess > 0, excess / (2.0 ** -24 * JJ), 0.0)
    return float(np.nan_to_num(k, nan=np.inf, posinf=np.inf).max())


def rodrigues(phi):
    phi = np.asarray(phi, np.float64)
    th = np.linalg.norm(phi)
    K = np.array([[0, -phi[2], phi[1]], [phi[2], 0, -phi[0]], [-phi[1], phi[0], 0]])
    if th == 0:
        return np.eye(3)
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


def finite_difference_j(cam, w2c, sc, dL=1e-3, eps=1e-6):
    """j_p by central differences of the arbiter's rendered sum_ch dL C_p under m_i -> exp(+-eps xi_k^) m_i (decisions of the
    unperturbed binary32 run held fixed), [H,W,6]"""
    f32, _, m64 = arbiter_forward(cam, w2c, sc)
    kw = dict(colors_precomp=sc["colors"], scales=sc["scales"], rotations=sc["rotations"])

    def render(m):
        f = ref.rasterize_forward(cam, np.ascontiguousarray(m), sc["opacities"], decisions=f32, **kw)
        return float(np.float32(dL)) * f["color"].sum(axis=0)

    W, H = cam.image_width, cam.image_height
    j = np.zeros((H, W, 6))
    for k in range(6):
        xi = np.zeros(6)
        xi[k] = eps
        outs = []
        for s in (1.0, -1.0):
            R = rodrigues(s * xi[3:])
            outs.append(render(m64 @ R.T + s * xi[:3]))
        j[:, :, k] = (outs[0] - outs[1]) / (2 * eps)
    return j
