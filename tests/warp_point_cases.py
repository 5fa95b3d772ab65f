"""An independent model of cvgs_warp_tables_from_points (include/cvgs_hip_ext.h) and the item sets its tests share.  numpy only: nothing
here imports the package or the oracle.

The similarity fit is Umeyama's SVD solution in float64 (what skimage's SimilarityTransform.estimate and insightface's estimate_norm
run) followed by np.linalg.inv; the three-point affine is np.linalg.solve.  The library computes the same transforms in closed form."""
import struct

import numpy as np

SIMILARITY, AFFINE3 = 0, 1
INVALID_M = (0.0, 0.0, -1.0, 0.0, 0.0, -1.0, 0.0, 0.0, 1.0)
# the five-point template recognisers are trained on (eyes, nose, mouth corners), inside 112 x 112
TMPL5 = np.array([[38.2946, 51.6963], [73.5318, 51.5014], [56.0252, 71.7366], [41.5493, 92.3655], [70.7299, 92.2041]], np.float32)
TMPL2 = TMPL5[:2].copy()
TMPL3 = TMPL5[:3].copy()
TMPL16 = np.array([[56.0 + 40.0 * np.cos(0.4 * i) * (1 + 0.02 * i), 56.0 + 30.0 * np.sin(0.4 * i)] for i in range(16)], np.float32)
# three corners of a 112 x 112 target: top-left, top-right, bottom-left
TMPL_BOX = np.array([[0.0, 0.0], [111.0, 0.0], [0.0, 111.0]], np.float32)


def entry_bytes(data, w, h, step, m, dw, dh):
    """One 64-byte table entry."""
    return struct.pack("<Q3i9f2i", int(data), w, h, step, *[float(v) for v in m], dw, dh)


def similarity_inverse(pts, tmpl):
    """pts [n, k, 2] (any float dtype), tmpl [k, 2] -> float64 [n, 3, 3]: Umeyama's least-squares similarity pts -> tmpl (no reflection),
    inverted."""
    p = np.asarray(pts, np.float64)
    q = np.asarray(tmpl, np.float64)
    n, k, _ = p.shape
    mp, mq = p.mean(axis=1), q.mean(axis=0)
    pc, qc = p - mp[:, None, :], q - mq
    A = np.einsum("ki,nkj->nij", qc, pc) / k              # dst^T src / k
    d = np.ones((n, 2))
    d[np.linalg.det(A) < 0, 1] = -1.0
    U, S, Vt = np.linalg.svd(A)
    # rank-deficient covariance (two landmarks, or collinear ones): its determinant is rounding noise, and Umeyama's rule takes the sign from
    # det(U) det(V) instead (np.linalg.matrix_rank's tolerance); the vanishing singular value leaves the scale alone either way
    deficient = S[:, 1] <= S[:, 0] * 2 * np.finfo(np.float64).eps
    dr = d.copy()
    dr[deficient, 1] = np.where(np.linalg.det(U[deficient]) * np.linalg.det(Vt[deficient]) > 0, 1.0, -1.0)
    R = np.einsum("nij,nj,njk->nik", U, dr, Vt)
    var = (pc ** 2).sum(axis=(1, 2)) / k
    scale = (S * d).sum(axis=1) / var
    M = np.zeros((n, 3, 3))
    M[:, :2, :2] = scale[:, None, None] * R
    M[:, :2, 2] = mq - np.einsum("nij,nj->ni", M[:, :2, :2], mp)
    M[:, 2, 2] = 1.0
    return np.linalg.inv(M)


def affine3_inverse(pts, tmpl):
    """pts [n, 3, 2], tmpl [3, 2] -> float64 [n, 3, 3]: the affine M with M (q_j, 1) = p_j."""
    p = np.asarray(pts, np.float64)
    Q = np.concatenate([np.asarray(tmpl, np.float64), np.ones((3, 1))], axis=1)  # rows (qx, qy, 1)
    Mt = np.linalg.solve(np.broadcast_to(Q, (len(p), 3, 3)), p)                  # Q M^T = P
    M = np.zeros((len(p), 3, 3))
    M[:, :2, :] = np.transpose(Mt, (0, 2, 1))
    M[:, 2, 2] = 1.0
    return M


def model_inverse(fit, pts, tmpl):
    return similarity_inverse(pts, tmpl) if fit == SIMILARITY else affine3_inverse(pts, tmpl)


def model_valid(fit, pts, count=None):
    """bool [n]: finite coordinates, (similarity) landmarks that do not all coincide, an index below the clamped count."""
    p = np.asarray(pts, np.float32)
    n = len(p)
    ok = np.isfinite(p).all(axis=(1, 2))
    if fit == SIMILARITY:
        ok &= ~(p == p[:, :1, :]).all(axis=(1, 2))
    live = n if count is None else min(max(int(count), 0), n)
    ok &= np.arange(n) < live
    return ok


def errors(table_m, model):
    """Per item: (largest error of a linear entry relative to the largest |linear entry| of the model, largest error of a translation
    entry relative to max(|that entry|, 1)).  table_m [n, 9] float32, model [n, 3, 3] float64."""
    m = np.asarray(table_m, np.float64).reshape(-1, 3, 3)
    lin = np.abs(m[:, :2, :2] - model[:, :2, :2]).max(axis=(1, 2)) / np.abs(model[:, :2, :2]).max(axis=(1, 2))
    tr = (np.abs(m[:, :2, 2] - model[:, :2, 2]) / np.maximum(np.abs(model[:, :2, 2]), 1.0)).max(axis=1)
    return lin, tr


def random_items(tmpl, n, seed, mirrored=False, noise=2.0):
    """float32 [n, k, 2]: the template under a random rotation (full circle), scale 0.2..6, translation 0..4000, plus Gaussian noise."""
    rng = np.random.default_rng(seed)
    q = np.asarray(tmpl, np.float64)
    if mirrored:
        q = q * np.array([-1.0, 1.0]) + np.array([112.0, 0.0])
    th = rng.uniform(0.0, 2.0 * np.pi, n)
    s = rng.uniform(0.2, 6.0, n)
    t = rng.uniform(0.0, 4000.0, (n, 2))
    R = np.stack([np.stack([np.cos(th), -np.sin(th)], -1), np.stack([np.sin(th), np.cos(th)], -1)], -2)
    p = s[:, None, None] * np.einsum("nij,kj->nki", R, q) + t[:, None, :] + rng.normal(0.0, noise, (n, len(q), 2))
    return p.astype(np.float32)


def random_affine_items(n, seed):
    """float32 [n, 3, 2]: three corners of oriented, sheared boxes."""
    rng = np.random.default_rng(seed)
    th = rng.uniform(0.0, 2.0 * np.pi, n)
    s = rng.uniform(0.2, 6.0, (n, 2))
    sh = rng.uniform(-0.3, 0.3, n)
    t = rng.uniform(0.0, 4000.0, (n, 2))
    L = np.stack([np.stack([s[:, 0] * np.cos(th), -s[:, 1] * np.sin(th) + sh * s[:, 0]], -1),
                  np.stack([s[:, 0] * np.sin(th), s[:, 1] * np.cos(th)], -1)], -2)
    p = np.einsum("nij,kj->nki", L, TMPL_BOX.astype(np.float64)) + t[:, None, :]
    return p.astype(np.float32)


def similarity_grid(n_main, n_side):
    """[(name, template, items)]: the 5-point grid plus K = 2, 3, 16 and a mirrored landmark set."""
    return [("k5", TMPL5, random_items(TMPL5, n_main, 1)), ("k2", TMPL2, random_items(TMPL2, n_side, 2)),
            ("k3", TMPL3, random_items(TMPL3, n_side, 3)), ("k16", TMPL16, random_items(TMPL16, n_side, 4)),
            ("k5_mirrored", TMPL5, random_items(TMPL5, n_side, 5, mirrored=True))]


def pinned_invalid(k, base=None):
    """float32 [m, k, 2] and bool [m] (valid under the SIMILARITY fit): NaN / +inf / -inf in each coordinate slot of an otherwise good
    item, coincident landmarks, and the good item itself."""
    good = (np.asarray(TMPL5 if base is None else base, np.float32)[:k] * np.float32(0.5) + np.float32(20.0)).astype(np.float32)
    items, valid = [good.copy()], [True]
    for bad in (np.nan, np.inf, -np.inf):
        for slot in range(2 * k):
            it = good.copy()
            it.reshape(-1)[slot] = bad
            items.append(it)
            valid.append(False)
    items.append(np.tile(np.array([[33.25, 17.5]], np.float32), (k, 1)))  # coincident landmarks
    valid.append(False)
    items.append(good.copy() + np.float32(1.0))
    valid.append(True)
    return np.stack(items), np.array(valid)
