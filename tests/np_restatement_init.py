"""NumPy restatement of the mono bootstrap's maths (no GPU, no C++): the checker of csrc/init.hip.

  * the homography estimator of include/svo_hip.h (svoh_homography_ransac_batch) -- an estimator of the project's own,
    because cv::findHomography cannot be restated; this file is its second, independent writing;
  * HomographyDecomp::removeScale + HomographyDecompInria::decompose (vikit/homography_decomp.h:121-126, 283-430);
  * the selection among the four motions of vk::estimateHomography (vikit_common/src/homography.cpp:88-135);
  * vk::triangulateFeatureNonLin, vk::computeInliers (vikit_common/src/math_utils.cpp:14-33, 66-98);
  * initialization_utils::triangulatePoints / rescaleAndInitializePoints (svo/src/initialization.cpp:756-840).
"""
import numpy as np

U64 = np.uint64
MAX_DRAWS, MAX_REFINE_ITERS = 64, 10
STATUS_OK, STATUS_NO_MODEL = 0, 1


# ---------------------------------------------------------------- estimator
def mix(x):
    """splitmix64's finaliser on uint64 arrays (arithmetic mod 2^64)."""
    with np.errstate(over="ignore"):
        x = np.asarray(x, U64) + U64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> U64(27))) * U64(0x94D049BB133111EB)
        return x ^ (x >> U64(31))


def sample_indices(seed, K, n):
    """(idx [K,4], ok [K]): the four different match indices of every hypothesis, ok = found within 64 draws."""
    h = np.arange(K, dtype=U64)
    kept = np.zeros((K, 4), np.int64)
    cnt = np.zeros(K, np.int64)
    for d in range(MAX_DRAWS):
        if np.all(cnt == 4):
            break
        with np.errstate(over="ignore"):
            r = (mix(U64(seed) ^ mix((h << U64(8)) + U64(d))) % U64(n)).astype(np.int64)
        seen = np.zeros(K, bool)
        for j in range(3):
            seen |= (cnt > j) & (kept[:, j] == r)
        take = (cnt < 4) & ~seen
        kept[take, cnt[take]] = r[take]
        cnt[take] += 1
    return kept, cnt == 4


def _basis(p):
    """p [K,4,3] homogeneous points -> (M [K,3,3] = [l1 p1, l2 p2, l3 p3] as columns, lam [K,3])."""
    p1, p2, p3, p4 = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
    lam = np.stack([np.einsum("ki,ki->k", np.cross(p2, p3), p4),
                    np.einsum("ki,ki->k", np.cross(p3, p1), p4),
                    np.einsum("ki,ki->k", np.cross(p1, p2), p4)], axis=1)
    M = np.stack([lam[:, 0, None] * p1, lam[:, 1, None] * p2, lam[:, 2, None] * p3], axis=2)
    return M, lam


def models_from_samples(uv_ref, uv_cur, idx):
    """(H [K,3,3] of Frobenius norm 1, ok [K], lam_gap): H = B adj(A) per hypothesis."""
    K = idx.shape[0]
    one = np.ones((K, 4, 1))
    with np.errstate(all="ignore"):
        A, la = _basis(np.concatenate([uv_ref[idx], one], axis=2))
        B, lb = _basis(np.concatenate([uv_cur[idx], one], axis=2))
        a1, a2, a3 = A[:, :, 0], A[:, :, 1], A[:, :, 2]
        adj = np.stack([np.cross(a2, a3), np.cross(a3, a1), np.cross(a1, a2)], axis=1)
        H = B @ adj
        norm = np.sqrt(np.sum(H * H, axis=(1, 2)))
        lmin = np.minimum(np.abs(la).min(axis=1), np.abs(lb).min(axis=1))   # NaN propagates
        ok = (lmin >= 1e-9) & (norm > 0) & np.isfinite(norm)
        H = H / norm[:, None, None]
        lam_gap = np.abs(lmin - 1e-9) / 1e-9
    return H, ok, lam_gap


def inlier_test(H, uv_ref, uv_cur, thresh):
    """H [...,3,3] -> (inlier [...,n], gap [...,n]); gap = | |e| - thresh|w| | / (thresh|w|), NaN where undefined."""
    with np.errstate(all="ignore"):
        pr = np.concatenate([uv_ref, np.ones((uv_ref.shape[0], 1))], axis=1)
        q = pr @ np.swapaxes(H, -1, -2)                     # [..., n, 3]
        x, y, w = q[..., 0], q[..., 1], q[..., 2]
        dx, dy = x - uv_cur[:, 0] * w, y - uv_cur[:, 1] * w
        e2, t2 = dx * dx + dy * dy, thresh * thresh * (w * w)
        inl = e2 < t2
        gap = np.abs(np.sqrt(e2) - np.sqrt(t2)) / np.sqrt(t2)
    return inl, gap


def refine(H, uv_ref, uv_cur, inl):
    """Gauss-Newton over the 8 free entries of H (H[2,2] = 1) on the matches `inl`.  Returns (H, iterations started)."""
    H = H.copy()
    u, v = uv_ref[inl, 0], uv_ref[inl, 1]
    uc, vc = uv_cur[inl, 0], uv_cur[inl, 1]
    iters = 0
    for _ in range(MAX_REFINE_ITERS):
        iters += 1
        with np.errstate(all="ignore"):
            x = H[0, 0] * u + H[0, 1] * v + H[0, 2]
            y = H[1, 0] * u + H[1, 1] * v + H[1, 2]
            w = H[2, 0] * u + H[2, 1] * v + H[2, 2]
            iw = 1.0 / w
            px, py = x * iw, y * iw
            z = np.zeros_like(u)
            Jx = np.stack([u * iw, v * iw, iw, z, z, z, -px * u * iw, -px * v * iw], axis=1)
            Jy = np.stack([z, z, z, u * iw, v * iw, iw, -py * u * iw, -py * v * iw], axis=1)
            A = Jx.T @ Jx + Jy.T @ Jy
            b = -(Jx.T @ (px - uc) + Jy.T @ (py - vc))
            try:
                dx = np.linalg.solve(A, b)
            except np.linalg.LinAlgError:
                dx = np.full(8, np.nan)
        if not np.all(np.isfinite(dx)):
            break
        H.ravel()[:8] += dx
        if np.abs(dx).max() < 1e-10:
            break
    return H, iters


def estimate_homography_ransac(uv_ref, uv_cur, thresh, seed, K=2000):
    """The estimator of svoh_homography_ransac_batch.  Returns a dict with the outputs of svoh_homography_result, the
    mask, and the gaps: the smallest relative distance of any error of any hypothesis to the threshold (gap_hyp), the
    same for the refined H (gap_final), and of any min|lambda| to its bound (gap_lambda)."""
    uv_ref = np.ascontiguousarray(uv_ref, np.float64).reshape(-1, 2)
    uv_cur = np.ascontiguousarray(uv_cur, np.float64).reshape(-1, 2)
    n = uv_ref.shape[0]
    out = dict(H=np.zeros((3, 3)), best_hypothesis=0, n_inliers_hypothesis=0, n_inliers=0, refine_iters=0,
               status=STATUS_NO_MODEL, mask=np.zeros(n, np.uint8), gap_hyp=np.inf, gap_final=np.inf, gap_lambda=np.inf)
    if n < 4 or K < 1:
        return out
    idx, sampled = sample_indices(seed, K, n)
    H, ok, lam_gap = models_from_samples(uv_ref, uv_cur, idx)
    ok &= sampled
    out["n_degenerate"] = int(np.sum(~ok))
    if np.any(sampled & np.isfinite(lam_gap)):
        out["gap_lambda"] = float(np.min(lam_gap[sampled & np.isfinite(lam_gap)]))
    if not np.any(ok):
        return out
    inl, gap = inlier_test(H, uv_ref, uv_cur, thresh)
    g = gap[ok]
    if np.any(np.isfinite(g)):
        out["gap_hyp"] = float(np.nanmin(g[np.isfinite(g)]))
    counts = np.where(ok, inl.sum(axis=1), -1)
    best = int(np.argmax(counts))          # the first of equals: the lowest h
    if counts[best] < 4:
        return out
    Hb, inl_b = H[best], inl[best]
    iters = 0
    if abs(Hb[2, 2]) >= 1e-12:
        Hb, iters = refine(Hb / Hb[2, 2], uv_ref, uv_cur, inl_b)
    mask, gap_f = inlier_test(Hb, uv_ref, uv_cur, thresh)
    if np.any(np.isfinite(gap_f)):
        out["gap_final"] = float(np.min(gap_f[np.isfinite(gap_f)]))
    out.update(H=Hb, best_hypothesis=best, n_inliers_hypothesis=int(counts[best]), n_inliers=int(mask.sum()),
               refine_iters=iters, status=STATUS_OK, mask=mask.astype(np.uint8))
    return out


# ---------------------------------------------------------------- decomposition (homography_decomp.h)
def _signd(x):
    return 1 if x >= 0 else -1


def _opposite_of_minor(M, row, col):
    x1 = 1 if col == 0 else 0
    x2 = 1 if col == 2 else 2
    y1 = 1 if row == 0 else 0
    y2 = 1 if row == 2 else 2
    return M[y1, x2] * M[y2, x1] - M[y1, x1] * M[y2, x2]


def decompose_homography(H):
    """cv::decomposeHomographyMat with K = I as the reference carries it: removeScale, then HomographyDecompInria.
    Returns a list of (R, t, n): four motions, or one (R, 0, 0) when H is a rotation up to 1e-3."""
    H = np.asarray(H, np.float64).reshape(3, 3)
    Hn = H * (1.0 / np.linalg.svd(H, compute_uv=False)[1])
    S = Hn.T @ Hn - np.eye(3)
    if np.abs(S).sum(axis=1).max() < 0.001:     # norm(S, NORM_INF) of a matrix: the largest absolute row sum
        return [(Hn.copy(), np.zeros(3), np.zeros(3))]
    M00, M11, M22 = _opposite_of_minor(S, 0, 0), _opposite_of_minor(S, 1, 1), _opposite_of_minor(S, 2, 2)
    with np.errstate(invalid="ignore"):
        rtM00, rtM11, rtM22 = np.sqrt(M00), np.sqrt(M11), np.sqrt(M22)
    M01, M12, M02 = _opposite_of_minor(S, 0, 1), _opposite_of_minor(S, 1, 2), _opposite_of_minor(S, 0, 2)
    e12, e02, e01 = _signd(M12), _signd(M02), _signd(M01)
    nS = [abs(S[0, 0]), abs(S[1, 1]), abs(S[2, 2])]
    indx = 0
    if nS[0] < nS[1]:
        indx = 1
        if nS[1] < nS[2]:
            indx = 2
    elif nS[0] < nS[2]:
        indx = 2
    if indx == 0:
        npa = np.array([S[0, 0], S[0, 1] + rtM22, S[0, 2] + e12 * rtM11])
        npb = np.array([S[0, 0], S[0, 1] - rtM22, S[0, 2] - e12 * rtM11])
    elif indx == 1:
        npa = np.array([S[0, 1] + rtM22, S[1, 1], S[1, 2] - e02 * rtM00])
        npb = np.array([S[0, 1] - rtM22, S[1, 1], S[1, 2] + e02 * rtM00])
    else:
        npa = np.array([S[0, 2] + e01 * rtM11, S[1, 2] + rtM00, S[2, 2]])
        npb = np.array([S[0, 2] - e01 * rtM11, S[1, 2] - rtM00, S[2, 2]])
    traceS = S[0, 0] + S[1, 1] + S[2, 2]
    with np.errstate(invalid="ignore"):
        v = 2.0 * np.sqrt(1 + traceS - M00 - M11 - M22)
        ESii = _signd(S[indx, indx])
        r = np.sqrt(2 + traceS + v)
        n_t = np.sqrt(2 + traceS - v)
        na, nb = npa / np.linalg.norm(npa), npb / np.linalg.norm(npb)
        half_nt, esii_t_r = 0.5 * n_t, ESii * r
        ta_star = half_nt * (esii_t_r * nb - n_t * na)
        tb_star = half_nt * (esii_t_r * na - n_t * nb)
        Ra = Hn @ (np.eye(3) - (2 / v) * np.outer(ta_star, na))
        Rb = Hn @ (np.eye(3) - (2 / v) * np.outer(tb_star, nb))
    ta, tb = Ra @ ta_star, Rb @ tb_star
    return [(Ra, ta, na), (Ra, -ta, -na), (Rb, tb, nb), (Rb, -tb, -nb)]


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], np.float64)


def sampson_distance(f_cur, E, f_ref):
    """vk::sampsonDistance for columns f_cur, f_ref [n,3]."""
    with np.errstate(all="ignore"):
        err = np.einsum("ni,ij,nj->n", f_cur, E, f_ref)
        pc, pr = f_ref @ E.T, f_cur @ E
        uc, ur = pc[:, :2] / pc[:, 2:3], pr[:, :2] / pr[:, 2:3]
        return err * err / (np.sum(uc * uc, axis=1) + np.sum(ur * ur, axis=1))


def select_motion(H, f_cur, f_ref, mask, thresh):
    """homography.cpp:64-135 after the inlier count.  Returns dict(R, t, n, score, cheirality [4], ok); ok False (and
    score 0) when the decomposition does not yield four motions -- the reference's CHECK_EQ would abort there."""
    motions = decompose_homography(H)
    if len(motions) != 4:
        return dict(ok=False, score=0.0, R=np.eye(3), t=np.zeros(3), n=np.zeros(3), cheirality=[])
    mask = np.asarray(mask, bool)
    cheir = [float(np.sum((f_cur[mask] @ n) > 0.0)) for (_, _, n) in motions]
    order = sorted(range(4), key=lambda i: -cheir[i])      # stable
    first, second = order[0], order[1]
    with np.errstate(all="ignore"):
        ratio = np.float64(cheir[second]) / np.float64(cheir[first])
    if ratio < 0.9:
        pick = first
    else:
        cap = thresh * thresh * 4.0
        s = []
        for i in (first, second):
            R, t, _ = motions[i]
            d = sampson_distance(f_cur, R @ skew(t), f_ref)
            with np.errstate(invalid="ignore"):
                d = np.where(cap < d, cap, d)               # std::min(d, cap): a NaN d stays
            s.append(float(np.sum(d)))
        pick = first if s[0] < s[1] else second
    R, t, n = motions[pick]
    return dict(ok=True, score=float(mask.sum()), R=R, t=t, n=n, cheirality=cheir, picked=pick)


# ---------------------------------------------------------------- triangulation (math_utils.cpp, initialization.cpp)
def triangulate_feature_nonlin(R, t, f1, f2):
    f2r = R @ f2
    b = np.array([t @ f1, t @ f2r])
    a10 = f1 @ f2r
    A = np.array([[f1 @ f1, -a10], [a10, -(f2r @ f2r)]])
    with np.errstate(all="ignore"):
        det = A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0]
        Ainv = np.array([[A[1, 1], -A[0, 1]], [-A[1, 0], A[0, 0]]]) / det
        lam = Ainv @ b
    return (lam[0] * f1 + t + lam[1] * f2r) / 2


def compute_inliers(f1, f2, R_12, t, reproj_thresh, error_multiplier2):
    """vk::computeInliers: indices j whose two reprojection errors are both <= reproj_thresh."""
    inliers = []
    for j in range(f1.shape[0]):
        X = triangulate_feature_nonlin(R_12, t, f1[j], f2[j])
        with np.errstate(all="ignore"):
            e1 = error_multiplier2 * np.linalg.norm(f1[j, :2] / f1[j, 2] - X[:2] / X[2])
            Y = R_12.T @ (X - t)
            e2 = error_multiplier2 * np.linalg.norm(f2[j, :2] / f2[j, 2] - Y[:2] / Y[2])
        if not (e1 > reproj_thresh or e2 > reproj_thresh):
            inliers.append(j)
    return inliers


def angle_error(f1, f2):
    with np.errstate(all="ignore"):
        return np.arccos((f1 @ f2) / (np.linalg.norm(f1) * np.linalg.norm(f2)))


def triangulate_points(f_cur, f_ref, R_cur_ref, t_cur_ref, angle_threshold, matches, pinhole=True):
    """initialization_utils::triangulatePoints: (kept matches, points_in_cur [m,3])."""
    kept, pts = [], []
    for (ic, ir) in matches:
        X = triangulate_feature_nonlin(R_cur_ref, t_cur_ref, f_cur[ic], f_ref[ir])
        e1 = angle_error(f_cur[ic], X)
        e2 = angle_error(f_ref[ir], R_cur_ref.T @ (X - t_cur_ref))
        if e1 > angle_threshold or e2 > angle_threshold or (pinhole and X[2] < 0.0):
            continue
        kept.append((ic, ir))
        pts.append(X)
    return kept, np.array(pts).reshape(-1, 3)


def rescale_and_initialize_points(points_in_cur, R_cur_ref, t_cur_ref, R_ref_w, t_ref_w, depth_at_current_frame):
    """initialization_utils::rescaleAndInitializePoints: (scale, R_cur_w, t_cur_w, points in world [m,3])."""
    depth = np.linalg.norm(points_in_cur, axis=1)
    median = np.sort(depth)[depth.size // 2]                 # vk::getMedian: the element at floor(n / 2)
    scale = depth_at_current_frame / median
    R_cur_w = R_cur_ref @ R_ref_w
    t_cur_w = R_cur_ref @ t_ref_w + t_cur_ref
    pos_ref, pos_cur = -R_ref_w.T @ t_ref_w, -R_cur_w.T @ t_cur_w
    t_cur_w = -R_cur_w @ (pos_ref + scale * (pos_cur - pos_ref))
    world = (points_in_cur * scale - t_cur_w) @ R_cur_w      # rows: R^T (p - t)
    return scale, R_cur_w, t_cur_w, world
