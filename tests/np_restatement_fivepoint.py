"""NumPy restatement of the essential-matrix estimator of include/svo_hip.h (svoh_essential_ransac_batch): the checker of
essential_ransac_kernel (csrc/essential.hip) and of the functions of csrc/svoh_essential.h.  The estimator is the project's
own (opengv's RANSAC cannot be restated); this file is its second, independent writing, vectorised over hypotheses where
the kernel loops, and it goes other ways where the definition leaves one: the null space by an SVD (optionally turned by
a fixed orthogonal 4 x 4), the elimination by a linear solve, the roots of the degree-10 polynomial as the eigenvalues of
its companion matrix (polished by Newton), (x, y) by an SVD, the motions of E by its SVD.  The score is the reference's
(TranslationSacProblemWithTriangulation::getSelectedDistancesToModel, src/svo/src/initialization.cpp:167-214)."""
import itertools

import numpy as np

from np_restatement_init import mix, U64

MAX_DRAWS, MAX_REFINE_ITERS, TINY, TINY_ELIMINATION, PARALLEL = 64, 10, 1e-12, 1e-9, 1e-12
STATUS_OK, STATUS_NO_MODEL = 0, 1

# monomials of (x, y, z) as exponent triples; degree <= 3 in the elimination's column order
_COLS3 = [(3, 0, 0), (0, 3, 0), (2, 1, 0), (1, 2, 0), (2, 0, 1), (2, 0, 0), (0, 2, 1), (0, 2, 0), (1, 1, 1), (1, 1, 0),
          (1, 0, 2), (1, 0, 1), (1, 0, 0), (0, 1, 2), (0, 1, 1), (0, 1, 0), (0, 0, 3), (0, 0, 2), (0, 0, 1), (0, 0, 0)]
_COLS1 = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
_COLS2 = sorted({tuple(a + b for a, b in zip(p, q)) for p in _COLS1 for q in _COLS1}, reverse=True)


def _product_table(left, right, out):
    T = np.zeros((len(left), len(right), len(out)))
    for (i, p), (j, q) in itertools.product(enumerate(left), enumerate(right)):
        T[i, j, out.index(tuple(a + b for a, b in zip(p, q)))] = 1.0
    return T


_T11 = _product_table(_COLS1, _COLS1, _COLS2)
_T21 = _product_table(_COLS2, _COLS1, _COLS3)


def sample_five(seed, K, n):
    """(idx [K,5], ok [K]): the five different match indices of every hypothesis, ok = found within 64 draws."""
    h = np.arange(K, dtype=U64)
    kept = np.zeros((K, 5), np.int64)
    cnt = np.zeros(K, np.int64)
    for d in range(MAX_DRAWS):
        if np.all(cnt == 5):
            break
        with np.errstate(over="ignore"):
            r = (mix(U64(seed) ^ mix((h << U64(8)) + U64(d))) % U64(n)).astype(np.int64)
        seen = np.zeros(K, bool)
        for j in range(4):
            seen |= (cnt > j) & (kept[:, j] == r)
        take = (cnt < 5) & ~seen
        kept[take, cnt[take]] = r[take]
        cnt[take] += 1
    return kept, cnt == 5


def polymul(a, b):
    """[..., da + 1] x [..., db + 1] -> [..., da + db + 1], lowest power first."""
    out = np.zeros(np.broadcast_shapes(a.shape[:-1], b.shape[:-1]) + (a.shape[-1] + b.shape[-1] - 1, ))
    for i in range(a.shape[-1]):
        for j in range(b.shape[-1]):
            out[..., i + j] += a[..., i] * b[..., j]
    return out


def polyval(p, x):
    """p [..., d + 1] lowest power first, x [...] (or [..., m] with p [..., None, d + 1])."""
    v = np.zeros_like(x) + p[..., -1]
    for i in range(p.shape[-1] - 2, -1, -1):
        v = v * x + p[..., i]
    return v


def essential_candidates(fc5, fr5, basis_turn=None):
    """fc5, fr5 [K,5,3] -> (E [K,10,3,3] with |E|_F^2 = 2, valid [K,10], degenerate [K], n_complex_near [K], smin [K]): the
    real solutions of every hypothesis in ascending order of the root (invalid ones last); smin: the smallest singular
    value of the elimination's left half (inf where the hypothesis was degenerate before).  The elimination is without a
    usable pivot when smin < 1e-9: the kernel's bound on its pivots, which are of smin's order."""
    K = fc5.shape[0]
    with np.errstate(all="ignore"):
        Q = np.einsum("ksi,ksj->ksij", fc5, fr5).reshape(K, 5, 9)
        bad = ~np.isfinite(Q).all(axis=(1, 2))
        Q[bad] = np.eye(9)[:5]
        _, sv, Vt = np.linalg.svd(Q)
        degenerate = bad | ~(sv[:, 4] >= TINY)
        basis = Vt[:, 5:, :]                                           # [K,4,9]: X, Y, Z, W
        if basis_turn is not None:
            basis = np.einsum("ab,kbe->kae", np.asarray(basis_turn, np.float64), basis)
        E1 = np.transpose(basis, (0, 2, 1)).reshape(K, 3, 3, 4)        # entry (i, j) as a polynomial of degree 1
        EEt = np.einsum("kiav,kjaw,vwm->kijm", E1, E1, _T11)
        lam = EEt - 0.5 * np.einsum("ij,km->kijm", np.eye(3), EEt[:, 0, 0] + EEt[:, 1, 1] + EEt[:, 2, 2])
        rows = np.einsum("kiam,kajv,mvq->kijq", lam, E1, _T21).reshape(K, 9, 20)
        det = np.zeros((K, 20))
        for j in range(3):
            j1, j2 = (j + 1) % 3, (j + 2) % 3
            cof = np.einsum("kv,kw,vwm->km", E1[:, 1, j1], E1[:, 2, j2], _T11) - np.einsum("kv,kw,vwm->km", E1[:, 1, j2], E1[:, 2, j1], _T11)
            det += np.einsum("km,kv,mvq->kq", cof, E1[:, 0, j], _T21)
        A = np.concatenate([rows, det[:, None, :]], axis=1)            # [K,10,20]
        left = A[:, :, :10].copy()
        smin = np.linalg.svd(np.where(degenerate[:, None, None], np.eye(10), left), compute_uv=False)[:, -1]
        smin = np.where(degenerate, np.inf, smin)
        degenerate |= ~(smin >= TINY_ELIMINATION)
        left[degenerate] = np.eye(10)
        Bm = np.linalg.solve(left, A[:, :, 10:])                       # rows 4..9: x^2z, x^2, y^2z, y^2, xyz, xy
        C = np.zeros((K, 3, 3, 5))                                     # row, (x, y, 1), power of z
        for r in range(3):
            hi, lo = Bm[:, 4 + 2 * r], Bm[:, 5 + 2 * r]
            for v in range(2):
                C[:, r, v, 0] = hi[:, 3 * v + 2]
                C[:, r, v, 1] = hi[:, 3 * v + 1] - lo[:, 3 * v + 2]
                C[:, r, v, 2] = hi[:, 3 * v + 0] - lo[:, 3 * v + 1]
                C[:, r, v, 3] = -lo[:, 3 * v + 0]
            C[:, r, 2, 0] = hi[:, 9]
            C[:, r, 2, 1] = hi[:, 8] - lo[:, 9]
            C[:, r, 2, 2] = hi[:, 7] - lo[:, 8]
            C[:, r, 2, 3] = hi[:, 6] - lo[:, 7]
            C[:, r, 2, 4] = -lo[:, 6]
        p = (polymul(polymul(C[:, 0, 0], C[:, 1, 1]) - polymul(C[:, 0, 1], C[:, 1, 0]), C[:, 2, 2])
             - polymul(polymul(C[:, 0, 0], C[:, 2, 1]) - polymul(C[:, 0, 1], C[:, 2, 0]), C[:, 1, 2])
             + polymul(polymul(C[:, 1, 0], C[:, 2, 1]) - polymul(C[:, 1, 1], C[:, 2, 0]), C[:, 0, 2]))[:, :11]
        monic = p[:, :10] / p[:, 10:11]
        degenerate |= ~np.isfinite(p).all(axis=1) | ~np.isfinite(monic).all(axis=1)
        monic[degenerate] = 0.0
        comp = np.zeros((K, 10, 10))
        comp[:, np.arange(1, 10), np.arange(0, 9)] = 1.0
        comp[:, :, 9] = -monic
        ev = np.linalg.eigvals(comp)                                   # [K,10] complex
        real = np.abs(ev.imag) <= 1e-8 * (1.0 + np.abs(ev.real))
        z = ev.real.copy()
        dp = p[:, 1:] * np.arange(1, 11)
        for _ in range(3):                                             # Newton on the real part
            zn = z - polyval(p[:, None, :], z) / polyval(dp[:, None, :], z)
            z = np.where(np.isfinite(zn) & real, zn, z)
        real &= ~degenerate[:, None]
        z = np.where(real, z, np.inf)
        order = np.argsort(z, axis=1, kind="stable")
        z = np.take_along_axis(z, order, axis=1)
        valid = np.take_along_axis(real, order, axis=1)
        zz = np.where(valid, z, 0.0)
        Mz = polyval(C[:, None, :, :, :], zz[:, :, None, None])        # [K,10,3,3]
        v = np.linalg.svd(Mz)[2][:, :, 2, :]                           # the right singular vector of the smallest value
        coef = np.stack([v[..., 0], v[..., 1], v[..., 2] * zz, v[..., 2]], axis=-1)   # [K,10,4]
        E = np.einsum("kcv,kve->kce", coef, basis)
        nn = np.einsum("kce,kce->kc", E, E)
        E = E * np.sqrt(2.0 / nn)[..., None]
        valid &= np.isfinite(E).all(axis=2) & (nn > 0)
        E = np.where(valid[..., None], E, 0.0).reshape(K, 10, 3, 3)
        near = ((np.abs(ev.imag) > 1e-8 * (1.0 + np.abs(ev.real))) & (np.abs(ev.imag) <= 1e-5 * (1.0 + np.abs(ev.real)))).sum(axis=1)
    return E, valid, degenerate, near, smin


def motions_of(E):
    """E [M,3,3] -> (R [M,4,3,3], t [M,4,3]): (R_a, t), (R_a, -t), (R_b, t), (R_b, -t) from the SVD of E."""
    with np.errstate(all="ignore"):
        U, _, Vt = np.linalg.svd(E)
        U = U * np.sign(np.linalg.det(U))[:, None, None]
        Vt = Vt * np.sign(np.linalg.det(Vt))[:, None, None]
        W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
        Ra, Rb = U @ W @ Vt, U @ W.T @ Vt
        t = U[:, :, 2]
    return np.stack([Ra, Ra, Rb, Rb], axis=1), np.stack([t, -t, t, -t], axis=1)


def errors(R, t, f_cur, f_ref):
    """R [M,3,3], t [M,3] -> (err [M,n], parallax [M,n]): midpoint triangulation in the current frame, then the two bearing
    errors; parallax = f.f g.g - (f.g)^2."""
    with np.errstate(all="ignore"):
        g = np.einsum("mij,nj->mni", R, f_ref)
        f = f_cur[None]
        c = np.einsum("mni,ni->mn", g, f_cur)
        ff = np.einsum("ni,ni->n", f_cur, f_cur)[None]
        gg = np.einsum("mni,mni->mn", g, g)
        det = c * c - ff * gg
        b0 = t @ f_cur.T
        b1 = np.einsum("mi,mni->mn", t, g)
        l0 = (-gg * b0 + c * b1) / det
        l1 = (-c * b0 + ff * b1) / det
        p = 0.5 * ((l0[..., None] * f + t[:, None, :]) + l1[..., None] * g)
        q = p - t[:, None, :]
        e1 = 1.0 - np.einsum("mni,mni->mn", p, np.broadcast_to(f, p.shape)) / np.sqrt(np.einsum("mni,mni->mn", p, p))
        e2 = 1.0 - np.einsum("mni,mni->mn", q, g) / np.sqrt(np.einsum("mni,mni->mn", q, q))
    return e1 + e2, -det


def inliers(R, t, f_cur, f_ref, thresh):
    err, par = errors(R, t, f_cur, f_ref)
    with np.errstate(all="ignore"):
        return (par >= PARALLEL) & (err < thresh)


def tangent(t):
    ax = 0
    for k in (1, 2):
        if abs(t[k]) < abs(t[ax]):
            ax = k
    a = np.zeros(3)
    a[ax] = 1.0
    b1 = np.cross(t, a)
    b1 /= np.sqrt(b1 @ b1)
    return b1, np.cross(t, b1)


def exp_so3(w):
    th = np.sqrt(w @ w)
    Wx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-8:
        A, B = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0
    else:
        A, B = np.sin(th) / th, (1.0 - np.cos(th)) / (th * th)
    return np.eye(3) + A * Wx + B * (Wx @ Wx)


def refine(R, t, f_cur, f_ref):
    """Gauss-Newton over (w, d1, d2) on the given matches.  Returns (R, t, iterations started, step sizes)."""
    steps = []
    iters = 0
    for _ in range(MAX_REFINE_ITERS):
        iters += 1
        b1, b2 = tangent(t)
        g = f_ref @ R.T
        u = np.cross(f_cur, t)
        r = np.einsum("ni,ni->n", u, g)
        jt = np.cross(g, f_cur)
        J = np.concatenate([np.cross(g, u), (jt @ b1)[:, None], (jt @ b2)[:, None]], axis=1)
        H, b = J.T @ J, -J.T @ r
        with np.errstate(all="ignore"):
            try:
                d = np.linalg.solve(H, b)
            except np.linalg.LinAlgError:
                d = np.full(5, np.nan)
        if not np.all(np.isfinite(d)):
            break
        steps.append(float(np.abs(d).max()))
        R = exp_so3(d[:3]) @ R
        t = t + b1 * d[3] + b2 * d[4]
        t = t / np.sqrt(t @ t)
        if steps[-1] < 1e-10:
            break
    return R, t, iters, steps


def estimate_essential_ransac(f_cur, f_ref, thresh, seed, K=2000, basis_turn=None):
    """The estimator of svoh_essential_ransac_batch.  Returns a dict with the outputs of svoh_essential_result, the mask,
    and what the premises of an exact comparison need: every scored candidate (cand_h, cand_c, cand_R, cand_t, cand_count),
    motion_unique (no candidate had two motions that hold its five), sample_err (the winner's five errors), R_winner,
    t_winner, steps (the refinement's step sizes), elim_smin (the smallest singular value of any elimination that was not degenerate)."""
    f_cur = np.ascontiguousarray(f_cur, np.float64).reshape(-1, 3)
    f_ref = np.ascontiguousarray(f_ref, np.float64).reshape(-1, 3)
    n = f_cur.shape[0]
    out = dict(R=np.zeros((3, 3)), t=np.zeros(3), best_hypothesis=0, best_candidate=0, n_inliers_hypothesis=0, n_inliers=0, n_degenerate=0,
               n_models=0, refine_iters=0, status=STATUS_NO_MODEL, mask=np.zeros(n, np.uint8), cand_h=np.zeros(0, np.int64),
               cand_c=np.zeros(0, np.int64), cand_R=np.zeros((0, 3, 3)), cand_t=np.zeros((0, 3)), cand_count=np.zeros(0, np.int64),
               motion_unique=True, elim_smin=np.inf, sample_err=np.zeros(5), R_winner=np.zeros((3, 3)), t_winner=np.zeros(3), steps=[])
    if n < 5 or K < 1:
        return out
    idx, sampled = sample_five(seed, K, n)
    fc5, fr5 = f_cur[idx], f_ref[idx]
    E, valid, degenerate, _, smin = essential_candidates(fc5, fr5, basis_turn)
    out["elim_smin"] = float(smin[smin >= TINY_ELIMINATION].min()) if np.any(smin >= TINY_ELIMINATION) else np.inf
    degenerate |= ~sampled
    valid &= ~degenerate[:, None]
    ch, cc = np.nonzero(valid)                                         # ascending h, then ascending root
    if len(ch) == 0:
        return out
    Rm, tm = motions_of(E[ch, cc])                                     # [M,4,3,3], [M,4,3]
    M = len(ch)
    passes = np.zeros((M, 4), bool)
    for m in range(4):
        for s in range(0, M, 4096):
            sl = slice(s, s + 4096)
            err, par = errors_per_row(Rm[sl, m], tm[sl, m], fc5[ch[sl]], fr5[ch[sl]])
            with np.errstate(all="ignore"):
                passes[sl, m] = ((par >= PARALLEL) & (err < thresh)).all(axis=1)
    out["motion_unique"] = bool((passes.sum(axis=1) <= 1).all())
    keep = passes.any(axis=1)
    first = np.argmax(passes, axis=1)
    ch, cc = ch[keep], cc[keep]
    cR, ct = Rm[keep, first[keep]], tm[keep, first[keep]]
    M = len(ch)
    if M == 0:
        return out
    counts = np.zeros(M, np.int64)
    slab = max(1, 200000 // max(n, 1))
    for s in range(0, M, slab):
        counts[s:s + slab] = inliers(cR[s:s + slab], ct[s:s + slab], f_cur, f_ref, thresh).sum(axis=1)
    out.update(cand_h=ch, cand_c=cc, cand_R=cR, cand_t=ct, cand_count=counts)
    best = int(np.argmax(counts))                                      # the first of the largest: lowest h, then lowest root
    if counts[best] < 5:
        return out
    R_win, t_win = cR[best], ct[best]
    err5, _ = errors_per_row(R_win[None], t_win[None], fc5[ch[best]][None], fr5[ch[best]][None])
    inl_win = inliers(R_win[None], t_win[None], f_cur, f_ref, thresh)[0]
    R_fin, t_fin, iters, steps = refine(R_win, t_win, f_cur[inl_win], f_ref[inl_win])
    inl = inliers(R_fin[None], t_fin[None], f_cur, f_ref, thresh)[0]
    out.update(R=R_fin, t=t_fin, best_hypothesis=int(ch[best]), best_candidate=int(cc[best]), n_inliers_hypothesis=int(counts[best]),
               n_inliers=int(inl.sum()), n_degenerate=int(degenerate.sum()), n_models=M, refine_iters=iters, status=STATUS_OK,
               mask=inl.astype(np.uint8), sample_err=err5[0], R_winner=R_win, t_winner=t_win, steps=steps)
    return out


def errors_per_row(R, t, f_cur, f_ref):
    """As errors, but with matches of its own for every model: f_cur, f_ref [M,s,3] -> [M,s]."""
    err = np.zeros(f_cur.shape[:2])
    par = np.zeros(f_cur.shape[:2])
    for s in range(f_cur.shape[1]):                                    # one sample position at a time, models vectorised
        e, p = _errors_diag(R, t, f_cur[:, s], f_ref[:, s])
        err[:, s], par[:, s] = e, p
    return err, par


def _errors_diag(R, t, f, fr):
    with np.errstate(all="ignore"):
        g = np.einsum("mij,mj->mi", R, fr)
        c = np.einsum("mi,mi->m", f, g)
        ff = np.einsum("mi,mi->m", f, f)
        gg = np.einsum("mi,mi->m", g, g)
        det = c * c - ff * gg
        b0 = np.einsum("mi,mi->m", t, f)
        b1 = np.einsum("mi,mi->m", t, g)
        l0 = (-gg * b0 + c * b1) / det
        l1 = (-c * b0 + ff * b1) / det
        p = 0.5 * ((l0[:, None] * f + t) + l1[:, None] * g)
        q = p - t
        e1 = 1.0 - np.einsum("mi,mi->m", p, f) / np.sqrt(np.einsum("mi,mi->m", p, p))
        e2 = 1.0 - np.einsum("mi,mi->m", q, g) / np.sqrt(np.einsum("mi,mi->m", q, q))
    return e1 + e2, -det
