"""fr_math.h's closed-form record rows (fr_mean_rows_unit) and identity-view projection (fr_preprocess_one<true>), compiled with
g++ into a harness of this test's own and compared on the CPU with the general chains they replace:
  * fr_mean_rows_unit<false, IDV> must give fr_mean_rows_g<false>'s rows bit for bit (a zero may change its sign, which == ignores),
    for the identity view (both instantiations) and for rigid non-identity views (IDV = false);
  * fr_preprocess_one<true> must give fr_preprocess_one<false>'s splat with an identity view bit for bit.
The inputs cover both fov clamps, needle-shaped splats and cov2D determinants near zero."""
import ctypes
import os

import numpy as np
import pytest

import harness_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fisher-nerf-customized_amd", "csrc")

SRC = r"""
#include "fr_math.h"
extern "C" {
// rows[n][2][15]: [0] = fr_mean_rows_g<false>, [1] = fr_mean_rows_unit<false, idv>
void rows(int n, const float* mean, const float* cov3D, const float* view, const float* proj, float fx, float fy, float tx, float ty,
          int W, int H, int idv, float* out)
{
	for (int i = 0; i < n; i++)
	{
		const fr_f3 m = { mean[3 * i], mean[3 * i + 1], mean[3 * i + 2] };
		const float* v = view + 16 * i;
		const float* pr = proj + 16 * i;
		float Rg[3][5], Ru[3][5];
		fr_mean_rows_g<false>(m, cov3D + 6 * i, v, pr, fx, fy, tx, ty, W, H, Rg, nullptr, nullptr, nullptr);
		if (idv) fr_mean_rows_unit<false, true>(m, cov3D + 6 * i, v, pr, fx, fy, tx, ty, W, H, Ru);
		else fr_mean_rows_unit<false, false>(m, cov3D + 6 * i, v, pr, fx, fy, tx, ty, W, H, Ru);
		memcpy(out + 30 * i, Rg, 60);
		memcpy(out + 30 * i + 15, Ru, 60);
	}
}
// splat[n][2][8]: {radius, depth, px, py, conx, cony, conz, rect x0 | y0 << 8 | x1 << 16 | y1 << 24} of fr_preprocess_one<false> with
// `view` and of fr_preprocess_one<true>
void splats(int n, const float* mean, const float* cov3D, const float* view, const float* proj, float fx, float fy, float tx, float ty,
            int W, int H, uint32_t gx, uint32_t gy, uint32_t* out)
{
	for (int i = 0; i < n; i++)
	{
		const fr_f3 m = { mean[3 * i], mean[3 * i + 1], mean[3 * i + 2] };
		const fr_splat s[2] = { fr_preprocess_one<false>(m, cov3D + 6 * i, view, proj + 16 * i, W, H, tx, ty, fx, fy, gx, gy),
		                        fr_preprocess_one<true>(m, cov3D + 6 * i, view, proj + 16 * i, W, H, tx, ty, fx, fy, gx, gy) };
		for (int k = 0; k < 2; k++)
		{
			uint32_t* o = out + 16 * i + 8 * k;
			o[0] = (uint32_t)s[k].radius; o[1] = fr_as_u32(s[k].depth + 0.f); o[2] = fr_as_u32(s[k].px + 0.f); o[3] = fr_as_u32(s[k].py + 0.f);
			o[4] = fr_as_u32(s[k].conx + 0.f); o[5] = fr_as_u32(s[k].cony + 0.f); o[6] = fr_as_u32(s[k].conz + 0.f);
			o[7] = s[k].rect.x0 | s[k].rect.y0 << 8 | s[k].rect.x1 << 16 | s[k].rect.y1 << 24;
		}
	}
}
}
"""

W, H = 256, 192
FX, FY = 180.0, 170.0
TX, TY = W / (2 * FX), H / (2 * FY)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("mean_rows_unit")
    src, so = d / "h.cpp", d / "h.so"
    src.write_text(SRC)
    harness_build.compile_shared(str(src), str(so), harness_build.EXACT + ("-fno-fast-math", f"-I{CSRC}"))
    return ctypes.CDLL(str(so))


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _rigid(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = rng.uniform(-1, 1, 3)
    return M


def _proj_cm(view_rm):
    """column-major full projection (clip = Pm @ view @ x, w = view-space z) and view matrix, as the raster settings hold them"""
    zn, zf = 0.01, 100.0
    Pm = np.array([[2 * FX / W, 0, 0, 0], [0, 2 * FY / H, 0, 0], [0, 0, zf / (zf - zn), -zf * zn / (zf - zn)], [0, 0, 1, 0]])
    return (Pm @ view_rm).T.reshape(16), view_rm.T.reshape(16)


def _cases(n, rng, identity):
    """camera-frame points / covariances of four families, the view of every case (identity or rigid), its full projection"""
    views = [np.eye(4) if identity else _rigid(rng) for _ in range(n)]
    fam = np.arange(n) % 4
    cam = np.empty((n, 3))
    cam[:, 2] = rng.uniform(0.05, 12.0, n)
    cam[:, 0] = rng.uniform(-1.0, 1.0, n) * TX * cam[:, 2]
    cam[:, 1] = rng.uniform(-1.0, 1.0, n) * TY * cam[:, 2]
    # family 1: outside the fov clamps, in x, in y or both (x_grad_mul / y_grad_mul = 0)
    f1 = fam == 1
    cam[f1, 0] *= rng.choice([1.0, 1.5, 3.0], f1.sum()) * rng.choice([-1, 1], f1.sum())
    cam[f1, 1] *= rng.choice([1.0, 1.6, 4.0], f1.sum())
    cam[f1 & (np.arange(n) % 8 == 1), 0] = 2.0 * TX * cam[f1 & (np.arange(n) % 8 == 1), 2]
    cam[f1 & (np.arange(n) % 8 == 5), 1] = -2.0 * TY * cam[f1 & (np.arange(n) % 8 == 5), 2]
    cov = np.empty((n, 6))
    for i in range(n):
        if fam[i] in (0, 1):                       # ordinary splats
            s = np.exp(rng.uniform(-5, -1, 3))
        elif fam[i] == 2:                          # needles: one axis 100 - 10^4 times the others
            s = np.exp(rng.uniform(-7, -5, 3))
            s[rng.integers(3)] *= 10 ** rng.uniform(2, 4)
        if fam[i] < 3:
            R = _rigid(rng)[:3, :3]
            S = R @ np.diag(s * s) @ R.T
        else:                                      # cov2D + 0.3 I near singular: det ~ 1e-4 .. 1e-9
            z = cam[i, 2]
            cam[i, :2] *= 1e-3
            e1, e2 = rng.uniform(0.01, 0.3, 2)
            e3 = np.sqrt(e1 * e2) * (1 - 10 ** rng.uniform(-8, -3)) * rng.choice([-1, 1])
            S = np.zeros((3, 3))
            S[0, 0] = (e1 - 0.3) * z * z / FX ** 2
            S[1, 1] = (e2 - 0.3) * z * z / FY ** 2
            S[0, 1] = S[1, 0] = e3 * z * z / (FX * FY)
            S[2, 2] = rng.uniform(1e-4, 1e-2)
        Rv = views[i][:3, :3]
        S = Rv.T @ S @ Rv                          # (given in the camera frame: the world-frame covariance)
        cov[i] = [S[0, 0], S[0, 1], S[0, 2], S[1, 1], S[1, 2], S[2, 2]]
    # world-frame means of the camera-frame points
    mean = np.stack([np.linalg.solve(views[i], np.append(cam[i], 1.0))[:3] for i in range(n)])
    pv = [_proj_cm(v) for v in views]
    proj = np.stack([p for p, _ in pv]).astype(np.float32)
    view = np.stack([v for _, v in pv]).astype(np.float32)
    return (np.ascontiguousarray(mean, np.float32), np.ascontiguousarray(cov, np.float32), np.ascontiguousarray(view),
            np.ascontiguousarray(proj), cam)


def _rows(lib, mean, cov, view, proj, idv):
    n = mean.shape[0]
    out = np.zeros((n, 2, 15), np.float32)
    lib.rows(ctypes.c_int(n), _p(mean), _p(cov), _p(view), _p(proj), ctypes.c_float(FX), ctypes.c_float(FY), ctypes.c_float(TX),
             ctypes.c_float(TY), ctypes.c_int(W), ctypes.c_int(H), ctypes.c_int(int(idv)), _p(out))
    return out[:, 0], out[:, 1]


@pytest.mark.parametrize("identity,idv", [(True, True), (True, False), (False, False)])
def test_closed_form_rows_equal_general_chain(lib, identity, idv):
    rng = np.random.default_rng(7 + 3 * identity + idv)
    mean, cov, view, proj, cam = _cases(4000, rng, identity)
    g, u = _rows(lib, mean, cov, view, proj, idv)
    assert np.isfinite(g).all()
    bad = np.nonzero(~(g == u).all(axis=1))[0]
    assert bad.size == 0, (bad[:5], g[bad[:2]], u[bad[:2]])
    # the families are what they claim: both clamps met, needles and near-singular determinants present
    tz = cam[:, 2]
    assert (np.abs(cam[:, 0] / tz) > 1.3 * TX).sum() > 100 and (np.abs(cam[:, 1] / tz) > 1.3 * TY).sum() > 100
    assert (np.abs(g[:, 10:15]) > 0).any(axis=1).mean() > 0.9


def test_identity_projection_bit_exact(lib):
    rng = np.random.default_rng(11)
    mean, cov, view, proj, _ = _cases(4000, rng, True)
    mean[::50, 2] = rng.uniform(0.0005, 0.002, mean[::50].shape[0])     # at the near plane
    n = mean.shape[0]
    out = np.zeros((n, 2, 8), np.uint32)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    lib.splats(ctypes.c_int(n), _p(mean), _p(cov), _p(view[0]), _p(proj), ctypes.c_float(FX), ctypes.c_float(FY), ctypes.c_float(TX),
               ctypes.c_float(TY), ctypes.c_int(W), ctypes.c_int(H), ctypes.c_uint32(gx), ctypes.c_uint32(gy), _p(out))
    assert np.array_equal(out[:, 0], out[:, 1])
    assert 0.3 * n < (out[:, 0, 0] > 0).sum() < n
