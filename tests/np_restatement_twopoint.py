"""NumPy restatement of the translation estimator of include/svo_hip.h (svoh_translation_ransac_batch): the checker of
translation_ransac_kernel (csrc/init.hip) and of the functions of csrc/svoh_translation.h.  The estimator is the project's own
(opengv's RANSAC cannot be restated); this file is its second, independent writing, vectorised over hypotheses where the
kernel loops.  The score is the reference's (TranslationSacProblemWithTriangulation::getSelectedDistancesToModel,
src/svo/src/initialization.cpp:167-214, on opengv's triangulate2)."""
import numpy as np

from np_restatement_init import mix, U64

MAX_DRAWS, JACOBI_SWEEPS, TINY = 64, 8, 1e-12
STATUS_OK, STATUS_NO_MODEL = 0, 1


def sample_pairs(seed, K, n):
    """(idx [K,2], ok [K]): the two different match indices of every hypothesis, ok = found within 64 draws."""
    h = np.arange(K, dtype=U64)
    kept = np.zeros((K, 2), np.int64)
    cnt = np.zeros(K, np.int64)
    for d in range(MAX_DRAWS):
        if np.all(cnt == 2):
            break
        with np.errstate(over="ignore"):
            r = (mix(U64(seed) ^ mix((h << U64(8)) + U64(d))) % U64(n)).astype(np.int64)
        take = (cnt == 0) | ((cnt == 1) & (kept[:, 0] != r))
        kept[take, cnt[take]] = r[take]
        cnt[take] += 1
    return kept, cnt == 2


def stage(f_cur, f_ref, R_cur_ref):
    """(g, m, Ainv [n,2,2]): the rotated reference bearings, f_cur x g, the inverse of A = [[f.f, -c], [c, -g.g]]."""
    with np.errstate(all="ignore"):
        g = f_ref @ np.asarray(R_cur_ref, np.float64).reshape(3, 3).T
        m = np.cross(f_cur, g)
        c = np.einsum("ni,ni->n", f_cur, g)
        ff = np.einsum("ni,ni->n", f_cur, f_cur)
        gg = np.einsum("ni,ni->n", g, g)
        idet = 1.0 / (c * c - ff * gg)
        Ainv = np.stack([np.stack([-gg * idet, c * idet], axis=1), np.stack([-c * idet, ff * idet], axis=1)], axis=1)
    return g, m, Ainv


def models_from_pairs(f_cur, g, m, idx):
    """(t [K,3] unit, ok [K], gap_norm, gap_sign): t = m_i x m_j, towards (f_cur_i - g_i); the gaps are the distances of
    |t| to 1e-12 (relative) and of the sign's dot product to zero (relative to |f_cur_i - g_i|)."""
    with np.errstate(all="ignore"):
        t = np.cross(m[idx[:, 0]], m[idx[:, 1]])
        norm = np.sqrt(np.einsum("ki,ki->k", t, t))
        ok = norm >= TINY
        t = t / norm[:, None]
        d = f_cur[idx[:, 0]] - g[idx[:, 0]]
        s = np.einsum("ki,ki->k", d, t)
        t = np.where((s < 0)[:, None], -t, t)
        gap_norm = np.abs(norm - TINY) / TINY
        gap_sign = np.abs(s) / np.sqrt(np.einsum("ki,ki->k", d, d))
    return t, ok, gap_norm, gap_sign


def errors(t, f_cur, g, Ainv):
    """t [...,3] -> err [...,n]: midpoint triangulation in the current frame, then the two bearing errors."""
    t = np.asarray(t, np.float64)
    with np.errstate(all="ignore"):
        b0 = t @ f_cur.T                                            # [..., n]
        b1 = t @ g.T
        l0 = Ainv[:, 0, 0] * b0 + Ainv[:, 0, 1] * b1
        l1 = Ainv[:, 1, 0] * b0 + Ainv[:, 1, 1] * b1
        p = 0.5 * ((l0[..., None] * f_cur + t[..., None, :]) + l1[..., None] * g)
        q = p - t[..., None, :]
        e1 = 1.0 - np.einsum("...ni,ni->...n", p, f_cur) / np.sqrt(np.einsum("...ni,...ni->...n", p, p))
        e2 = 1.0 - np.einsum("...ni,ni->...n", q, g) / np.sqrt(np.einsum("...ni,...ni->...n", q, q))
    return e1 + e2


def inlier_test(t, f_cur, g, Ainv, thresh):
    """(inlier [...,n], gap [...,n]); gap = |err - thresh| / thresh, NaN where the error is."""
    err = errors(t, f_cur, g, Ainv)
    with np.errstate(all="ignore"):
        return err < thresh, np.abs(err - thresh) / thresh


def moment_matrix(m, inl):
    """M = sum mhat mhat^T over the matches `inl` with |m| >= 1e-12."""
    mm = m[inl]
    norm = np.sqrt(np.einsum("ni,ni->n", mm, mm))
    keep = norm >= TINY
    mh = mm[keep] / norm[keep, None]
    return mh.T @ mh


def jacobi_smallest_eigenvector(M):
    """The unit eigenvector of the smallest eigenvalue of a symmetric 3x3 matrix: 8 sweeps of cyclic Jacobi over the
    pairs (0,1), (0,2), (1,2); a pair whose entry is exactly zero is passed over; the first among equal eigenvalues."""
    A = np.array(M, np.float64).copy()
    V = np.eye(3)
    with np.errstate(all="ignore"):
        for _ in range(JACOBI_SWEEPS):
            for p, q in ((0, 1), (0, 2), (1, 2)):
                if A[p, q] == 0.0:
                    continue
                theta = (A[q, q] - A[p, p]) / (2.0 * A[p, q])
                tn = (1.0 if theta >= 0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(tn * tn + 1.0)
                s = tn * c
                J = np.eye(3)
                J[p, p] = c; J[q, q] = c; J[p, q] = s; J[q, p] = -s
                A = J.T @ (A @ J)
                V = V @ J
        e = np.diag(A)
        k = 0
        for i in (1, 2):
            if e[i] < e[k]:
                k = i
        v = V[:, k]
        return v / np.sqrt(v @ v)


def refine(M, t_winner):
    v = jacobi_smallest_eigenvector(M)
    if not np.all(np.isfinite(v)):
        return np.array(t_winner, np.float64)
    return v if v @ t_winner >= 0.0 else -v


def estimate_translation_ransac(f_cur, f_ref, R_cur_ref, thresh, seed, K=2000):
    """The estimator of svoh_translation_ransac_batch.  Returns a dict with the outputs of svoh_translation_result, the
    mask, and what the premises of an exact comparison need: gap_hyp / gap_final (the smallest relative distance of any
    error of any hypothesis / of the final model to the threshold), gap_norm, gap_sign (models_from_pairs), tie_ok (the
    winner's count is unique or tied only with higher h), eig_gap ((lambda_mid - lambda_min) / lambda_max of M),
    t_winner, M."""
    f_cur = np.ascontiguousarray(f_cur, np.float64).reshape(-1, 3)
    f_ref = np.ascontiguousarray(f_ref, np.float64).reshape(-1, 3)
    n = f_cur.shape[0]
    out = dict(t=np.zeros(3), best_hypothesis=0, n_inliers_hypothesis=0, n_inliers=0, n_degenerate=0, status=STATUS_NO_MODEL,
               mask=np.zeros(n, np.uint8), gap_hyp=np.inf, gap_final=np.inf, gap_norm=np.inf, gap_sign=np.inf, tie_ok=True,
               eig_gap=np.inf, t_winner=np.zeros(3))
    if n < 2 or K < 1:
        return out
    g, m, Ainv = stage(f_cur, f_ref, R_cur_ref)
    idx, sampled = sample_pairs(seed, K, n)
    t, ok, gap_norm, gap_sign = models_from_pairs(f_cur, g, m, idx)
    fin = sampled & np.isfinite(gap_norm)
    if np.any(fin):
        out["gap_norm"] = float(gap_norm[fin].min())
    ok &= sampled
    if not np.any(ok):
        return out
    out["gap_sign"] = float(np.nanmin(gap_sign[ok])) if np.any(np.isfinite(gap_sign[ok])) else np.inf
    counts = np.full(K, -1, np.int64)
    gap_hyp = np.inf
    hs = np.flatnonzero(ok)
    for a in range(0, len(hs), 256):                                  # in slabs: [256, n, 3] temporaries
        sl = hs[a:a + 256]
        inl, gap = inlier_test(t[sl], f_cur, g, Ainv, thresh)
        counts[sl] = inl.sum(axis=1)
        if np.any(np.isfinite(gap)):
            gap_hyp = min(gap_hyp, float(gap[np.isfinite(gap)].min()))
    out["gap_hyp"] = gap_hyp
    best = int(np.argmax(counts))                                      # the first of the largest: the lowest h
    if counts[best] < 2:
        return out
    out["tie_ok"] = not np.any(counts[:best] == counts[best])          # (true by construction; kept as the premise states it)
    t_win = t[best]
    inl_win, _ = inlier_test(t_win, f_cur, g, Ainv, thresh)
    M = moment_matrix(m, inl_win)
    lam = np.sort(np.linalg.eigvalsh(M))
    out["eig_gap"] = float((lam[1] - lam[0]) / lam[2]) if lam[2] > 0 else 0.0
    t_fin = refine(M, t_win)
    inl, gap = inlier_test(t_fin, f_cur, g, Ainv, thresh)
    if np.any(np.isfinite(gap)):
        out["gap_final"] = float(gap[np.isfinite(gap)].min())
    out.update(t=t_fin, best_hypothesis=best, n_inliers_hypothesis=int(counts[best]), n_inliers=int(inl.sum()),
               n_degenerate=int(np.sum(~ok)), status=STATUS_OK, mask=inl.astype(np.uint8), t_winner=t_win, M=M)
    return out
