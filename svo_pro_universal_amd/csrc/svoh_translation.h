// svoh_translation.h -- the per-hypothesis maths of the translation estimator (include/svo_hip.h,
// svoh_translation_ransac_batch; DESIGN.md, "TwoPoint initialiser") as functions host and device code share: a staged
// match, the model from two matches, the error of one match (the reference's
// TranslationSacProblemWithTriangulation::getSelectedDistancesToModel, src/svo/src/initialization.cpp:167-214, on
// opengv's triangulate2), the count of a model over staged columns, and the eigenvector of the refinement.
// csrc/init.hip runs them in translation_ransac_kernel; tests/cpp_twopoint runs them serially on the CPU.
#pragma once

#include "svoh_math.h"

namespace svoh {

// a staged match: f_cur[3], g[3] = R_cur_ref f_ref, then the three different entries of A^-1 (rule 4):
// A = [[f.f, -c], [c, -g.g]], c = f.g, A^-1 = [[-g.g, c], [-c, f.f]] / (c c - f.f g.g)
constexpr int kTranslationCols = 9;
constexpr int kTranslationMaxDraws = 64;
constexpr int kTranslationJacobiSweeps = 8;   // a 3x3 symmetric matrix is diagonal to rounding after 4 - 5
constexpr double kTranslationTiny = 1e-12;

SVOH_HD double tr_dot(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
SVOH_HD void tr_cross(const double a[3], const double b[3], double out[3])
{
  out[0] = a[1] * b[2] - a[2] * b[1];
  out[1] = a[2] * b[0] - a[0] * b[2];
  out[2] = a[0] * b[1] - a[1] * b[0];
}
SVOH_HD bool tr_finite(double v) { return fabs(v) <= DBL_MAX; }
// 1 / sqrt(s) for the two normalisations of the score.  On the device: the hardware's reciprocal square root as a seed and
// two Newton steps (to a few 1e-16) instead of an fp64 square root and an fp64 division, which were two thirds of the
// scoring loop's instructions.  s = 0, infinite or a NaN gives a NaN (0 times infinity in the step): no inlier either way.
SVOH_HD double tr_rsqrt(double s)
{
#if defined(__HIP_DEVICE_COMPILE__)
  const double hs = 0.5 * s;
  double r = __builtin_amdgcn_rsq(s);
  r = r * (1.5 - hs * (r * r));
  r = r * (1.5 - hs * (r * r));
  return r;
#else
  return 1.0 / sqrt(s);
#endif
}

SVOH_HD unsigned long long translation_mix(unsigned long long x)
{
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// rule 2: the two different match indices of hypothesis h; false when 64 draws do not hold two
SVOH_HD bool translation_sample(unsigned long long seed, unsigned h, unsigned n, unsigned& i, unsigned& j)
{
  int kept = 0;
  i = j = 0;
  for (int d = 0; d < kTranslationMaxDraws && kept < 2; ++d) {
    const unsigned long long r = translation_mix(seed ^ translation_mix(((unsigned long long)h << 8) + (unsigned long long)d));
    const unsigned idx = (unsigned)(r % n);
    if (kept == 0) { i = idx; kept = 1; }
    else if (idx != i) { j = idx; kept = 2; }
  }
  return kept == 2;
}

// rule 1 (and the part of rule 4 that does not depend on the model)
SVOH_HD void translation_stage(const double R[9], const double f_cur[3], const double f_ref[3], double col[kTranslationCols])
{
  double g[3];
  for (int r = 0; r < 3; ++r) g[r] = R[3 * r] * f_ref[0] + R[3 * r + 1] * f_ref[1] + R[3 * r + 2] * f_ref[2];
  const double c = tr_dot(f_cur, g), ff = tr_dot(f_cur, f_cur), gg = tr_dot(g, g);
  const double idet = 1.0 / (c * c - ff * gg);   // not finite for parallel rays: such a match is never an inlier
  for (int k = 0; k < 3; ++k) { col[k] = f_cur[k]; col[3 + k] = g[k]; }
  col[6] = -gg * idet;
  col[7] = c * idet;
  col[8] = ff * idet;
}

// rule 3: t from the matches i and j (f: f_cur, g: the rotated f_ref); false = degenerate
SVOH_HD bool translation_from_two(const double fi[3], const double gi[3], const double fj[3], const double gj[3], double t[3])
{
  double mi[3], mj[3];
  tr_cross(fi, gi, mi);
  tr_cross(fj, gj, mj);
  tr_cross(mi, mj, t);
  const double norm = sqrt(tr_dot(t, t));
  if (!(norm >= kTranslationTiny)) return false;   // also a NaN
  const double d[3] = { fi[0] - gi[0], fi[1] - gi[1], fi[2] - gi[2] };
  for (int k = 0; k < 3; ++k) t[k] /= norm;
  if (tr_dot(d, t) < 0.0) { t[0] = -t[0]; t[1] = -t[1]; t[2] = -t[2]; }
  return true;
}

// rule 4: midpoint triangulation in the current frame, then the two bearing errors; a0, a1, a2 = the staged A^-1
SVOH_HD double translation_error(const double t[3], double f0, double f1, double f2, double g0, double g1, double g2, double a0, double a1,
                                 double a2)
{
  const double b0 = t[0] * f0 + t[1] * f1 + t[2] * f2;
  const double b1 = t[0] * g0 + t[1] * g1 + t[2] * g2;
  const double l0 = a0 * b0 + a1 * b1, l1 = a2 * b1 - a1 * b0;
  const double p0 = 0.5 * ((l0 * f0 + t[0]) + l1 * g0), p1 = 0.5 * ((l0 * f1 + t[1]) + l1 * g1), p2 = 0.5 * ((l0 * f2 + t[2]) + l1 * g2);
  const double q0 = p0 - t[0], q1 = p1 - t[1], q2 = p2 - t[2];
  const double e1 = 1.0 - (f0 * p0 + f1 * p1 + f2 * p2) * tr_rsqrt(p0 * p0 + p1 * p1 + p2 * p2);
  const double e2 = 1.0 - (g0 * q0 + g1 * q1 + g2 * q2) * tr_rsqrt(q0 * q0 + q1 * q1 + q2 * q2);
  return e1 + e2;
}

// match i of columns laid out as cols[k * cap + i], k < kTranslationCols
SVOH_HD bool translation_is_inlier(const double t[3], const double* cols, int cap, int i, double thresh)
{
  return translation_error(t, cols[i], cols[cap + i], cols[2 * cap + i], cols[3 * cap + i], cols[4 * cap + i], cols[5 * cap + i], cols[6 * cap + i],
                           cols[7 * cap + i], cols[8 * cap + i]) < thresh;   // false for a NaN
}

// the scoring stage: a model in, its count out (another model of the relative pose scores the same way)
SVOH_HD int translation_count_inliers(const double t[3], const double* cols, int cap, int n, double thresh)
{
  int count = 0;
  for (int i = 0; i < n; ++i) count += translation_is_inlier(t, cols, cap, i, thresh) ? 1 : 0;
  return count;
}

// rule 6, one match's part of M = sum mhat mhat^T (xx, xy, xz, yy, yz, zz); nothing for |m| < 1e-12
SVOH_HD void translation_accumulate(const double* cols, int cap, int i, double acc[6])
{
  const double f[3] = { cols[i], cols[cap + i], cols[2 * cap + i] }, g[3] = { cols[3 * cap + i], cols[4 * cap + i], cols[5 * cap + i] };
  double m[3];
  tr_cross(f, g, m);
  const double norm = sqrt(tr_dot(m, m));
  if (!(norm >= kTranslationTiny)) return;
  const double x = m[0] / norm, y = m[1] / norm, z = m[2] / norm;
  acc[0] += x * x; acc[1] += x * y; acc[2] += x * z; acc[3] += y * y; acc[4] += y * z; acc[5] += z * z;
}

// rule 6: the unit eigenvector of M's smallest eigenvalue by cyclic Jacobi, a fixed number of sweeps (a pair whose
// off-diagonal entry is exactly zero is passed over); among equal eigenvalues the first
SVOH_HD void translation_smallest_eigenvector(const double M[6], double v[3])
{
  double A[3][3] = { { M[0], M[1], M[2] }, { M[1], M[3], M[4] }, { M[2], M[4], M[5] } };
  double V[3][3] = { { 1, 0, 0 }, { 0, 1, 0 }, { 0, 0, 1 } };
#if defined(__HIPCC__)
#pragma unroll 1
#endif
  for (int sweep = 0; sweep < kTranslationJacobiSweeps; ++sweep) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int pq = 0; pq < 3; ++pq) {
      const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;   // (0, 1), (0, 2), (1, 2)
      if (A[p][q] == 0.0) continue;
      const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
      const double tn = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
      const double c = 1.0 / sqrt(tn * tn + 1.0), s = tn * c;
      for (int k = 0; k < 3; ++k) {   // A <- A J
        const double akp = A[k][p], akq = A[k][q];
        A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq;
      }
      for (int k = 0; k < 3; ++k) {   // A <- J^T A
        const double apk = A[p][k], aqk = A[q][k];
        A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk;
      }
      for (int k = 0; k < 3; ++k) {   // V <- V J
        const double vkp = V[k][p], vkq = V[k][q];
        V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq;
      }
    }
  }
  const double e0 = A[0][0], e1 = A[1][1], e2 = A[2][2];
  double x = V[0][0], y = V[1][0], z = V[2][0], e = e0;
  if (e1 < e) { x = V[0][1]; y = V[1][1]; z = V[2][1]; e = e1; }
  if (e2 < e) { x = V[0][2]; y = V[1][2]; z = V[2][2]; }
  const double norm = sqrt(x * x + y * y + z * z);
  v[0] = x / norm; v[1] = y / norm; v[2] = z / norm;
}

// rule 6's end: the refined t from M and the winner's t
SVOH_HD void translation_refine(const double M[6], const double t_winner[3], double t[3])
{
  double v[3];
  translation_smallest_eigenvector(M, v);
  if (!(tr_finite(v[0]) && tr_finite(v[1]) && tr_finite(v[2]))) { t[0] = t_winner[0]; t[1] = t_winner[1]; t[2] = t_winner[2]; return; }
  const double sgn = tr_dot(v, t_winner) >= 0.0 ? 1.0 : -1.0;
  t[0] = sgn * v[0]; t[1] = sgn * v[1]; t[2] = sgn * v[2];
}

}  // namespace svoh
