// svoh_essential.h -- the per-hypothesis maths of the essential-matrix estimator (include/svo_hip.h,
// svoh_essential_ransac_batch; DESIGN.md, "FivePoint initialiser") as functions host and device code share: the sample of
// five, the minimal solver (Nister's route: a four-dimensional null space, ten cubic constraints, an elimination, a
// polynomial of degree ten in one unknown, its real roots between the roots of its derivatives), the four motions of an
// essential matrix in closed form, the score of svoh_translation.h with the rotation applied per match, and one match's
// part of the Gauss-Newton refinement.  csrc/essential.hip runs them in essential_ransac_kernel; tests/cpp_fivepoint runs
// them serially on the CPU.  The solver's working set (a 10 x 20 matrix among it) lives in per-thread local arrays.
#pragma once

#include "svoh_translation.h"

// the solver's large steps are functions of their own on the device: inlined into the kernel their unrolled
// arithmetic competes with the scoring loop for the lane's registers
#if defined(__HIPCC__)
#define SVOH_HD_CALL __host__ __device__ __noinline__
#else
#define SVOH_HD_CALL inline
#endif

namespace svoh {

constexpr int kEssentialCols = 6;             // a staged match: f_cur[3], f_ref[3]
constexpr int kEssentialMaxDraws = 64;
constexpr int kEssentialMaxRoots = 10;
constexpr int kEssentialBisections = 64;     // halvings of an interval of ordered bit patterns: down to neighbouring doubles
constexpr int kEssentialNAcc = 15 + 5;        // packed lower triangle of J^T J, then -J^T r
constexpr double kEssentialTiny = 1e-12;
constexpr double kEssentialTinyPivot = 1e-9;  // the elimination's pivots: a camera that only turned leaves them at rounding's size
constexpr double kEssentialParallel = 1e-12;  // rule 4: |f_cur x g|^2 below this (rays within 1e-6 rad) is no inlier

// ---- polynomials in (x, y, z, 1): the variables are numbered 0 .. 3, a monomial is a sorted tuple of them ----
// degree 2: xx xy xz x yy yz y zz z 1;  degree 3: xxx xxy xxz xx xyy xyz xy xzz xz x yyy yyz yy yzz yz y zzz zz z 1
SVOH_HD int es_idx2(int i, int j)
{
  if (i > j) { const int s = i; i = j; j = s; }
  return 4 * i - i * (i - 1) / 2 + (j - i);
}
SVOH_HD int es_idx3(int i, int j, int k)
{
  if (i > j) { const int s = i; i = j; j = s; }
  if (j > k) { const int s = j; j = k; k = s; }
  if (i > j) { const int s = i; i = j; j = s; }
  const int off = i == 0 ? 0 : (i == 1 ? 10 : (i == 2 ? 16 : 19));
  const int m = 4 - i, dj = j - i;
  return off + dj * m - dj * (dj - 1) / 2 + (k - j);
}
// out (degree 2) += s * a * b, a and b of degree 1
SVOH_HD void es_mul11(const double* a, const double* b, double s, double* out)
{
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) out[es_idx2(i, j)] += s * a[i] * b[j];
}
// out (degree 3) += s * a * b, a of degree 2, b of degree 1
SVOH_HD void es_mul21(const double* a, const double* b, double s, double* out)
{
  for (int i = 0; i < 4; ++i)
    for (int j = i; j < 4; ++j) {
      const double aij = s * a[es_idx2(i, j)];
      for (int k = 0; k < 4; ++k) out[es_idx3(i, j, k)] += aij * b[k];
    }
}
// the column of a cubic monomial in the elimination's order:
// x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1
SVOH_HD int es_column(int monomial)
{
  switch (monomial) {
    case 0: return 0;   case 10: return 1;  case 1: return 2;   case 4: return 3;   case 2: return 4;
    case 3: return 5;   case 11: return 6;  case 12: return 7;  case 5: return 8;   case 6: return 9;
    case 7: return 10;  case 8: return 11;  case 9: return 12;  case 13: return 13; case 14: return 14;
    case 15: return 15; case 16: return 16; case 17: return 17; case 18: return 18; default: return 19;
  }
}

// rule 1: the five different match indices of hypothesis h; false when 64 draws do not hold five
SVOH_HD bool essential_sample(unsigned long long seed, unsigned h, unsigned n, unsigned idx[5])
{
  int kept = 0;
  for (int k = 0; k < 5; ++k) idx[k] = 0;
  for (int d = 0; d < kEssentialMaxDraws && kept < 5; ++d) {
    const unsigned long long r = translation_mix(seed ^ translation_mix(((unsigned long long)h << 8) + (unsigned long long)d));
    const unsigned i = (unsigned)(r % n);
    bool seen = false;
    for (int k = 0; k < 5; ++k) seen = seen || (k < kept && idx[k] == i);
    if (!seen) {
      for (int k = 0; k < 5; ++k) if (k == kept) idx[k] = i;
      ++kept;
    }
  }
  return kept == 5;
}

// A fixed orthogonal 4 x 4 (the left product of the quaternion (1, 2, 4, 10) / 11 times the right product of (2, 3, 6, 0) / 7;
// no entry is zero): essential_turn_basis takes a basis in special position to one in general position (essential_solve).
SVOH_HD double essential_turn(int i, int j)
{
  const int num[16] = { -28, -67, 16, -20, -53, 20, -44, -28, 44, -4, -16, -61, 20, -32, -59, 32 };
  return (double)num[4 * i + j] / 77.0;
}
SVOH_HD void essential_turn_basis(double B[4][9])
{
#if defined(__HIPCC__)
#pragma unroll 1
#endif
  for (int e = 0; e < 9; ++e) {
    const double b[4] = { B[0][e], B[1][e], B[2][e], B[3][e] };
    for (int i = 0; i < 4; ++i) B[i][e] = essential_turn(i, 0) * b[0] + essential_turn(i, 1) * b[1] + essential_turn(i, 2) * b[2] + essential_turn(i, 3) * b[3];
  }
}

// rule 2, first step: an orthonormal basis B[4][9] of the null space of the five rows q = f_cur (x) f_ref (row-major E);
// Gauss-Jordan with full pivoting, then modified Gram-Schmidt, then the fixed turn.  false: no usable pivot.
SVOH_HD_CALL bool essential_nullspace(const double fs[5][6], double B[4][9])
{
  double A[5][9];
  int perm[9];
  for (int c = 0; c < 9; ++c) perm[c] = c;
  for (int r = 0; r < 5; ++r)
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) A[r][3 * i + j] = fs[r][i] * fs[r][3 + j];
#if defined(__HIPCC__)
#pragma unroll 1
#endif
  for (int k = 0; k < 5; ++k) {
    int pr = k, pc = k;
    double big = -1.0;
    for (int r = k; r < 5; ++r)
      for (int c = k; c < 9; ++c) {
        const double v = fabs(A[r][c]);
        if (v > big) { big = v; pr = r; pc = c; }
      }
    if (!(big >= kEssentialTiny) || !tr_finite(big)) return false;
    for (int c = 0; c < 9; ++c) { const double s = A[k][c]; A[k][c] = A[pr][c]; A[pr][c] = s; }
    for (int r = 0; r < 5; ++r) { const double s = A[r][k]; A[r][k] = A[r][pc]; A[r][pc] = s; }
    { const int s = perm[k]; perm[k] = perm[pc]; perm[pc] = s; }
    const double ip = 1.0 / A[k][k];
    for (int c = 0; c < 9; ++c) A[k][c] *= ip;
    for (int r = 0; r < 5; ++r) {
      if (r == k) continue;
      const double m = A[r][k];
      for (int c = 0; c < 9; ++c) A[r][c] -= m * A[k][c];
    }
  }
  for (int j = 0; j < 4; ++j) {
    for (int c = 0; c < 9; ++c) B[j][c] = 0.0;
    B[j][perm[5 + j]] = 1.0;
    for (int r = 0; r < 5; ++r) B[j][perm[r]] = -A[r][5 + j];
  }
  for (int j = 0; j < 4; ++j) {
    for (int i = 0; i < j; ++i) {
      double d = 0.0;
      for (int c = 0; c < 9; ++c) d += B[i][c] * B[j][c];
      for (int c = 0; c < 9; ++c) B[j][c] -= d * B[i][c];
    }
    double nn = 0.0;
    for (int c = 0; c < 9; ++c) nn += B[j][c] * B[j][c];
    const double in = 1.0 / sqrt(nn);
    for (int c = 0; c < 9; ++c) B[j][c] *= in;
  }
  essential_turn_basis(B);
  return true;
}

// rule 2, second step: E = x B0 + y B1 + z B2 + B3; det E = 0 and E E^T E - tr(E E^T) E / 2 = 0 as ten rows over the twenty
// cubic monomials, reduced on their first ten columns by Gauss-Jordan with row pivoting; out: rows 4 .. 9 of the right half
// (the rows that lead with x^2z, x^2, y^2z, y^2, xyz, xy).  false: no usable pivot.
SVOH_HD_CALL bool essential_eliminate(const double B[4][9], double Bt[6][10])
{
  double A[10][20];
  for (int r = 0; r < 10; ++r)
    for (int c = 0; c < 20; ++c) A[r][c] = 0.0;
  {
    double E[9][4];   // entry e as a polynomial of degree 1
    for (int e = 0; e < 9; ++e)
      for (int v = 0; v < 4; ++v) E[e][v] = B[v][e];
    double EEt[6][10];   // 00 01 02 11 12 22
    double tr[10];
    for (int m = 0; m < 10; ++m) tr[m] = 0.0;
    {
      int s = 0;
      for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j, ++s) {
          for (int m = 0; m < 10; ++m) EEt[s][m] = 0.0;
          for (int k = 0; k < 3; ++k) es_mul11(E[3 * i + k], E[3 * j + k], 1.0, EEt[s]);
          if (i == j)
            for (int m = 0; m < 10; ++m) tr[m] += 0.5 * EEt[s][m];
        }
    }
    for (int d = 0; d < 3; ++d) {
      const int s = d == 0 ? 0 : (d == 1 ? 3 : 5);
      for (int m = 0; m < 10; ++m) EEt[s][m] -= tr[m];
    }
    double p3[20];
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (int i = 0; i < 3; ++i) {
#if defined(__HIPCC__)
#pragma unroll 1
#endif
      for (int j = 0; j < 3; ++j) {
        for (int m = 0; m < 20; ++m) p3[m] = 0.0;
        for (int k = 0; k < 3; ++k) {
          const int a = i < k ? i : k, b = i < k ? k : i;
          const int s = a == 0 ? b : (a == 1 ? 2 + b : 5);
          es_mul21(EEt[s], E[3 * k + j], 1.0, p3);
        }
        for (int m = 0; m < 20; ++m) A[3 * i + j][es_column(m)] = p3[m];
      }
    }
    // det E along the first row
    for (int m = 0; m < 20; ++m) p3[m] = 0.0;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (int j = 0; j < 3; ++j) {
      const int j1 = (j + 1) % 3, j2 = (j + 2) % 3;
      double cof[10];
      for (int m = 0; m < 10; ++m) cof[m] = 0.0;
      es_mul11(E[3 + j1], E[6 + j2], 1.0, cof);
      es_mul11(E[3 + j2], E[6 + j1], -1.0, cof);
      es_mul21(cof, E[j], 1.0, p3);
    }
    for (int m = 0; m < 20; ++m) A[9][es_column(m)] = p3[m];
  }
#if defined(__HIPCC__)
#pragma unroll 1
#endif
  for (int k = 0; k < 10; ++k) {
    int pr = k;
    double big = -1.0;
    for (int r = k; r < 10; ++r) {
      const double v = fabs(A[r][k]);
      if (v > big) { big = v; pr = r; }
    }
    if (!(big >= kEssentialTinyPivot) || !tr_finite(big)) return false;
    for (int c = k; c < 20; ++c) { const double s = A[k][c]; A[k][c] = A[pr][c]; A[pr][c] = s; }
    const double ip = 1.0 / A[k][k];
    for (int c = k; c < 20; ++c) A[k][c] *= ip;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (int r = 0; r < 10; ++r) {
      if (r == k) continue;
      const double m = A[r][k];
      for (int c = k; c < 20; ++c) A[r][c] -= m * A[k][c];
    }
  }
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 10; ++c) Bt[r][c] = A[4 + r][10 + c];
  return true;
}

// rule 2, third step: the three rows (x p3(z) + y p3(z) + p4(z) = 0) left when z times the row of x^2 (y^2, xy) is taken
// from the row of x^2z (y^2z, xyz); C[row][0..3]: the cubic of x, [4..7]: of y, [8..12]: the quartic; lowest power first
SVOH_HD void essential_rows_in_z(const double Bt[6][10], double C[3][13])
{
  for (int r = 0; r < 3; ++r) {
    const double* hi = Bt[2 * r];       // leads with ... z
    const double* lo = Bt[2 * r + 1];   // the same without z
    for (int v = 0; v < 2; ++v) {
      C[r][4 * v + 0] = hi[3 * v + 2];
      C[r][4 * v + 1] = hi[3 * v + 1] - lo[3 * v + 2];
      C[r][4 * v + 2] = hi[3 * v + 0] - lo[3 * v + 1];
      C[r][4 * v + 3] = -lo[3 * v + 0];
    }
    C[r][8] = hi[9];
    C[r][9] = hi[8] - lo[9];
    C[r][10] = hi[7] - lo[8];
    C[r][11] = hi[6] - lo[7];
    C[r][12] = -lo[6];
  }
}

// the determinant of those three rows: p[0 .. 10], lowest power first
SVOH_HD void essential_polynomial(const double C[3][13], double p[11])
{
  for (int k = 0; k < 11; ++k) p[k] = 0.0;
  for (int r = 0; r < 3; ++r) {
    const int r1 = r == 0 ? 1 : 0, r2 = r == 2 ? 1 : 2;   // the other two rows, ascending
    const double sgn = r == 1 ? -1.0 : 1.0;
    double minor[7];
    for (int k = 0; k < 7; ++k) minor[k] = 0.0;
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) minor[i + j] += C[r1][i] * C[r2][4 + j] - C[r1][4 + i] * C[r2][j];
    for (int i = 0; i < 7; ++i)
      for (int j = 0; j < 5; ++j) p[i + j] += sgn * minor[i] * C[r][8 + j];
  }
}

SVOH_HD double es_horner(const double* q, int deg, double x)
{
  double v = q[deg];
  for (int i = deg - 1; i >= 0; --i) v = v * x + q[i];
  return v;
}

// doubles as integers in the doubles' order (-0 and +0 are one), and back: the midpoint of two such integers is a
// bisection step whose 64 repetitions separate any two doubles, whatever their magnitudes
SVOH_HD long long es_ordered(double x)
{
  const long long b = __builtin_bit_cast(long long, x);
  return b < 0 ? -(b & 0x7FFFFFFFFFFFFFFFll) : b;
}
SVOH_HD double es_unordered(long long k)
{
  return k < 0 ? -__builtin_bit_cast(double, -k) : __builtin_bit_cast(double, k);
}

// rule 2, fourth step: the real roots of p in ascending order.  The roots of the (10 - d)-th derivative, d = 1 .. 10, each
// sought between neighbouring roots of the derivative before it (and the Cauchy bound at both ends), where the polynomial is
// monotonic: a sign change is bisected 64 times on the ordered bit patterns of the doubles, which ends at two neighbouring
// doubles; the root is the one with the smaller |value|.  -1: a coefficient or the bound is not finite.
SVOH_HD_CALL int essential_real_roots(const double p[11], double roots[kEssentialMaxRoots])
{
  double big = 0.0;
  bool finite = true;
  for (int i = 0; i <= 10; ++i) finite = finite && tr_finite(p[i]);
  for (int i = 0; i < 10; ++i) big = fmax(big, fabs(p[i] / p[10]));
  const double bound = 1.0 + big;
  if (!finite || !tr_finite(bound)) return -1;
  double prev[kEssentialMaxRoots], q[11];
  int n_prev = 0;
  for (int i = 0; i < kEssentialMaxRoots; ++i) prev[i] = roots[i] = 0.0;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
  for (int deg = 1; deg <= 10; ++deg) {
    const int k = 10 - deg;
    for (int i = 0; i <= 10; ++i) {
      double fall = 1.0;   // (i + k)! / i!
      for (int m = 1; m <= 10; ++m) if (m <= k) fall *= (double)(i + m);
      q[i] = i <= deg ? p[i + k] * fall : 0.0;
    }
    int n_cur = 0;
    double lo = -bound, flo = es_horner(q, deg, lo);
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (int j = 0; j <= n_prev; ++j) {
      const double hi = j < n_prev ? prev[j] : bound, fhi = es_horner(q, deg, hi);
      if ((flo < 0.0) != (fhi < 0.0)) {
        long long a = es_ordered(lo), b = es_ordered(hi);
        const bool rising = flo < 0.0;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
        for (int it = 0; it < kEssentialBisections; ++it) {
          const long long mid = (a >> 1) + (b >> 1) + (a & b & 1);
          const bool below = (es_horner(q, deg, es_unordered(mid)) < 0.0) == rising;
          a = below ? mid : a;
          b = below ? b : mid;
        }
        const double xa = es_unordered(a), xb = es_unordered(b);
        const double x = fabs(es_horner(q, deg, xa)) <= fabs(es_horner(q, deg, xb)) ? xa : xb;
        if (n_cur < kEssentialMaxRoots) roots[n_cur++] = x;
      }
      lo = hi; flo = fhi;
    }
    n_prev = n_cur;
    for (int i = 0; i < kEssentialMaxRoots; ++i) prev[i] = roots[i];
  }
  return n_prev;
}

// rule 2, last step: the essential matrix of a root, |E|_F^2 = 2; false: not finite or zero
SVOH_HD bool essential_from_root(const double C[3][13], const double B[4][9], double z, double E[9])
{
  double M[3][3];
  for (int r = 0; r < 3; ++r) {
    M[r][0] = es_horner(C[r], 3, z);
    M[r][1] = es_horner(C[r] + 4, 3, z);
    M[r][2] = es_horner(C[r] + 8, 4, z);
  }
  double v[3] = { 0, 0, 0 }, vn = -1.0;
  for (int pq = 0; pq < 3; ++pq) {   // (0, 1), (0, 2), (1, 2): the largest cross product, the first among equals
    const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
    double w[3];
    tr_cross(M[p], M[q], w);
    const double nn = tr_dot(w, w);
    if (nn > vn) { vn = nn; v[0] = w[0]; v[1] = w[1]; v[2] = w[2]; }
  }
  const double cx = v[0], cy = v[1], cz = v[2] * z, cw = v[2];
  double nn = 0.0;
  for (int e = 0; e < 9; ++e) {
    E[e] = cx * B[0][e] + cy * B[1][e] + cz * B[2][e] + cw * B[3][e];
    nn += E[e] * E[e];
  }
  const double s = sqrt(2.0 / nn);
  if (!(nn > 0.0) || !tr_finite(s)) return false;
  for (int e = 0; e < 9; ++e) E[e] *= s;
  return true;
}

// R <- R (3 I - R^T R) / 2, five times: the rotation nearest to an R that is one to rounding or to the accuracy of an
// ill-conditioned root; false when what is left is further than 1e-9 from orthogonal (or a NaN)
SVOH_HD bool es_orthonormalise(double R[9])
{
  double M[9];
#if defined(__HIPCC__)
#pragma unroll 1
#endif
  for (int it = 0; it <= 5; ++it) {
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) M[3 * i + j] = (i == j ? 3.0 : 0.0) - (R[i] * R[j] + R[3 + i] * R[3 + j] + R[6 + i] * R[6 + j]);
    if (it == 5) break;
    double Rn[9];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) Rn[3 * i + j] = 0.5 * (R[3 * i] * M[j] + R[3 * i + 1] * M[3 + j] + R[3 * i + 2] * M[6 + j]);
    for (int k = 0; k < 9; ++k) R[k] = Rn[k];
  }
  double worst = 0.0;
  bool finite = true;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double e = fabs(M[3 * i + j] - (i == j ? 2.0 : 0.0));
      finite = finite && tr_finite(e);
      worst = fmax(worst, e);
    }
  return finite && worst < 1e-9;
}

// rule 3: E (|E|_F^2 = 2) = [t]x Ra = [-t]x Rb.  t: the largest cross product of two columns (the first among equals),
// normalised; with the cofactor matrix Cof(E) = t t^T R: Ra = Cof(E) - [t]x E, Rb = Cof(E) + [t]x E, each made orthonormal.
SVOH_HD bool essential_motions(const double E[9], double Ra[9], double Rb[9], double t[3])
{
  const double c[3][3] = { { E[0], E[3], E[6] }, { E[1], E[4], E[7] }, { E[2], E[5], E[8] } };
  double tn = -1.0;
  t[0] = t[1] = t[2] = 0.0;
  for (int pq = 0; pq < 3; ++pq) {
    const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
    double w[3];
    tr_cross(c[p], c[q], w);
    const double nn = tr_dot(w, w);
    if (nn > tn) { tn = nn; t[0] = w[0]; t[1] = w[1]; t[2] = w[2]; }
  }
  const double norm = sqrt(tn);
  if (!(norm >= kEssentialTiny) || !tr_finite(norm)) return false;
  for (int k = 0; k < 3; ++k) t[k] /= norm;
  double cof[3][3];
  tr_cross(E + 3, E + 6, cof[0]);
  tr_cross(E + 6, E, cof[1]);
  tr_cross(E, E + 3, cof[2]);
  for (int j = 0; j < 3; ++j) {
    double te[3];
    tr_cross(t, c[j], te);
    for (int i = 0; i < 3; ++i) { Ra[3 * i + j] = cof[i][j] - te[i]; Rb[3 * i + j] = cof[i][j] + te[i]; }
  }
  const bool oka = es_orthonormalise(Ra), okb = es_orthonormalise(Rb);
  return oka && okb;
}

// rule 4: svoh_translation.h's error with g = R f_ref and the 2x2 inverse of this match; parallel rays are no inlier
SVOH_HD bool essential_is_inlier(const double R[9], const double t[3], double f0, double f1, double f2, double r0, double r1, double r2,
                                 double thresh)
{
  const double g0 = R[0] * r0 + R[1] * r1 + R[2] * r2, g1 = R[3] * r0 + R[4] * r1 + R[5] * r2, g2 = R[6] * r0 + R[7] * r1 + R[8] * r2;
  const double c = f0 * g0 + f1 * g1 + f2 * g2, ff = f0 * f0 + f1 * f1 + f2 * f2, gg = g0 * g0 + g1 * g1 + g2 * g2;
  const double det = c * c - ff * gg;
  const double idet = 1.0 / det;
  const double err = translation_error(t, f0, f1, f2, g0, g1, g2, -gg * idet, c * idet, ff * idet);
  return (-det >= kEssentialParallel) && (err < thresh);   // false for a NaN
}
SVOH_HD bool essential_is_inlier(const double R[9], const double t[3], const double* cols, int cap, int i, double thresh)
{
  return essential_is_inlier(R, t, cols[i], cols[cap + i], cols[2 * cap + i], cols[3 * cap + i], cols[4 * cap + i], cols[5 * cap + i], thresh);
}
// the scoring stage: a model in, its count out
SVOH_HD int essential_count_inliers(const double R[9], const double t[3], const double* cols, int cap, int n, double thresh)
{
  int count = 0;
  for (int i = 0; i < n; ++i) count += essential_is_inlier(R, t, cols, cap, i, thresh) ? 1 : 0;
  return count;
}

// rule 2 as one call: the five staged matches in, the null-space basis, the three rows in z and the real roots out; the number
// of roots, or -1 for a degenerate hypothesis.  The elimination singles out the basis: its left block has no usable pivot, the
// polynomial no leading coefficient, or the wanted root is one of a cluster, when a solution lies at or near infinity of
// (x, y, z) or a basis vector is itself an essential matrix.  The basis of essential_nullspace has a one and three zeros in
// every vector and so inherits the zeros of E = [t]x: on exact matches of a camera that did not turn it is in such a special
// position for every fifth sample.  That is a property of the basis, not of the five matches, so essential_nullspace turns
// its basis by the fixed orthogonal matrix: general position for any data that is not built from that matrix.  A camera that
// only turned has no usable pivot in any basis.
SVOH_HD_CALL int essential_solve(const double fs[5][6], double B[4][9], double C[3][13], double roots[kEssentialMaxRoots])
{
  double p[11];
  {
    double Bt[6][10];
    if (!essential_nullspace(fs, B)) return -1;
    if (!essential_eliminate(B, Bt)) return -1;
    essential_rows_in_z(Bt, C);
  }
  essential_polynomial(C, p);
  return essential_real_roots(p, roots);
}

// rule 3 as one call: the motion of the candidate at root z, the first of the four that holds the five; false: dropped
SVOH_HD_CALL bool essential_candidate(const double C[3][13], const double B[4][9], double z, const double fs[5][6], double thresh, double R[9],
                                      double t[3])
{
  double E[9], Ra[9], Rb[9], tc[3];
  if (!essential_from_root(C, B, z, E)) return false;
  if (!essential_motions(E, Ra, Rb, tc)) return false;
  int pick = -1;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
  for (int m = 3; m >= 0; --m) {   // (Ra, +t), (Ra, -t), (Rb, +t), (Rb, -t): the first that holds the five
    double Rm[9];
    for (int k = 0; k < 9; ++k) Rm[k] = m < 2 ? Ra[k] : Rb[k];
    const double sg = (m & 1) ? -1.0 : 1.0;
    const double tm[3] = { sg * tc[0], sg * tc[1], sg * tc[2] };
    bool all = true;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (int s = 0; s < 5; ++s) all = all && essential_is_inlier(Rm, tm, fs[s][0], fs[s][1], fs[s][2], fs[s][3], fs[s][4], fs[s][5], thresh);
    pick = all ? m : pick;
  }
  if (pick < 0) return false;
  for (int k = 0; k < 9; ++k) R[k] = pick < 2 ? Ra[k] : Rb[k];
  for (int k = 0; k < 3; ++k) t[k] = (pick & 1) ? -tc[k] : tc[k];
  return true;
}

// rules 1 - 4 for hypothesis h.  false: degenerate.  Else n_models candidates were scored; when there is one, count,
// candidate (its position among the real roots, ascending), R and t are those of the best (the first among equals).
SVOH_HD bool essential_hypothesis(unsigned long long seed, unsigned h, const double* cols, int cap, int n, double thresh, int& n_models,
                                  int& count, int& candidate, double R[9], double t[3])
{
  n_models = 0;
  count = -1;
  candidate = 0;
  unsigned idx[5];
  if (!essential_sample(seed, h, (unsigned)n, idx)) return false;
  double fs[5][6];
  for (int s = 0; s < 5; ++s)
    for (int k = 0; k < 6; ++k) fs[s][k] = cols[k * cap + (int)idx[s]];
  double B[4][9], C[3][13], roots[kEssentialMaxRoots];
  const int n_roots = essential_solve(fs, B, C, roots);
  if (n_roots < 0) return false;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
  for (int c = 0; c < n_roots; ++c) {
    double Rm[9], tm[3];
    if (!essential_candidate(C, B, roots[c], fs, thresh, Rm, tm)) continue;
    const int cnt = essential_count_inliers(Rm, tm, cols, cap, n, thresh);
    ++n_models;
    if (cnt > count) {
      count = cnt;
      candidate = c;
      for (int k = 0; k < 9; ++k) R[k] = Rm[k];
      for (int k = 0; k < 3; ++k) t[k] = tm[k];
    }
  }
  return true;
}

// rule 6: the basis of t's tangent plane
SVOH_HD void essential_tangent(const double t[3], double b1[3], double b2[3])
{
  int ax = 0;
  if (fabs(t[1]) < fabs(t[ax])) ax = 1;
  if (fabs(t[2]) < fabs(t[ax])) ax = 2;
  const double a[3] = { ax == 0 ? 1.0 : 0.0, ax == 1 ? 1.0 : 0.0, ax == 2 ? 1.0 : 0.0 };
  tr_cross(t, a, b1);
  const double in = 1.0 / sqrt(tr_dot(b1, b1));
  for (int k = 0; k < 3; ++k) b1[k] *= in;
  tr_cross(t, b1, b2);
}

// rule 6, one match's part of the 15 + 5 sums: r = f_cur . (t x g), dr/dw = g x (f_cur x t), dr/dd_k = (g x f_cur) . b_k
SVOH_HD void essential_accumulate(const double R[9], const double t[3], const double b1[3], const double b2[3], const double* cols, int cap,
                                  int i, double acc[kEssentialNAcc])
{
  const double f[3] = { cols[i], cols[cap + i], cols[2 * cap + i] }, fr[3] = { cols[3 * cap + i], cols[4 * cap + i], cols[5 * cap + i] };
  double g[3], u[3], jw[3], jt[3];
  for (int r = 0; r < 3; ++r) g[r] = R[3 * r] * fr[0] + R[3 * r + 1] * fr[1] + R[3 * r + 2] * fr[2];
  tr_cross(f, t, u);
  tr_cross(g, u, jw);
  tr_cross(g, f, jt);
  const double res = tr_dot(u, g);
  const double J[5] = { jw[0], jw[1], jw[2], tr_dot(jt, b1), tr_dot(jt, b2) };
  for (int r = 0; r < 5; ++r) {
    for (int c = 0; c <= r; ++c) acc[r * (r + 1) / 2 + c] += J[r] * J[c];
    acc[15 + r] -= J[r] * res;
  }
}

// rule 6: R <- Exp(w) R, t <- normalise(t + b1 d1 + b2 d2) for the step d = (w, d1, d2)
SVOH_HD void essential_update(const double d[5], const double b1[3], const double b2[3], double R[9], double t[3])
{
  const double th2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2], th = sqrt(th2);
  const double A = th < 1e-8 ? 1.0 - th2 / 6.0 : sin(th) / th, Bc = th < 1e-8 ? 0.5 - th2 / 24.0 : (1.0 - cos(th)) / th2;
  double Rn[9];
  for (int j = 0; j < 3; ++j) {
    const double col[3] = { R[j], R[3 + j], R[6 + j] };
    double w1[3], w2[3];
    tr_cross(d, col, w1);
    tr_cross(d, w1, w2);
    for (int i = 0; i < 3; ++i) Rn[3 * i + j] = col[i] + A * w1[i] + Bc * w2[i];
  }
  for (int k = 0; k < 9; ++k) R[k] = Rn[k];
  double tn[3];
  for (int k = 0; k < 3; ++k) tn[k] = t[k] + b1[k] * d[3] + b2[k] * d[4];
  const double in = 1.0 / sqrt(tr_dot(tn, tn));
  for (int k = 0; k < 3; ++k) t[k] = tn[k] * in;
}

}  // namespace svoh
