// init.hip -- the estimators of the mono bootstrap, each a batch of RANSAC problems with one workgroup of 256 threads per
// problem: the homography ("Homography initialiser"; below) and the translation under a known rotation
// ("TwoPoint initialiser"; translation_ransac_kernel, in the file's second half).
//
// The reference calls cv::findHomography(..., cv::RANSAC, thresh) (vikit_common/src/homography.cpp:36-43), whose random
// numbers, early stop and polish are OpenCV's.  This is an estimator of our own, a function of its inputs alone:
//   1. hypothesis h draws match indices from a counter-based generator (splitmix64 of seed and (h << 8) + d) until it has
//      four different ones, 64 draws at the most;
//   2. the model from four pairs in closed form: H = B adj(A), with A and B the matrices that send the projective basis
//      to the four ref and cur points;
//   3. every one of the K hypotheses is scored on every match (dx^2 + dy^2 < thresh^2 w^2); the winner has the largest
//      count, the lowest h among equals;
//   4. Gauss-Newton over the 8 free entries of H / H[8] on the winner's inliers, normal equations in fp64;
//   5. the mask and count of homography.cpp:47-56 with the refined H.
// The matches of a problem lie in LDS as four columns of doubles; in the scoring loop all lanes of a wave read the same
// match (one address: a broadcast), each lane with a hypothesis of its own in registers.  No global atomics, nothing
// shared between workgroups, no waiting; every loop is bounded by n, K, 64 or 10.
#include <cmath>
#include <cstring>
#include <vector>

#include "svoh_internal.h"
#include "svoh_device_utils.h"
#include "svoh_translation.h"

namespace svoh {

namespace {

constexpr int kInitThreads = 256;
constexpr int kInitWaves = kInitThreads / 64;
constexpr int kInitMaxMatches = 1024;   // 4 columns x 1024 x 8 bytes = 32 KB of LDS
constexpr int kInitMaxDraws = 64;
constexpr int kInitMaxRefineIters = 10;
constexpr int kInitNAcc = 36 + 8;       // packed lower triangle of J^T J, then -J^T r

struct InitProblemDev {
  double thresh;
  unsigned long long seed;
  int32_t n;
  int32_t first;        // the problem's first match in the mask array; its columns start at double 4 * first
  int32_t pad_[2];
};

struct InitArgs {
  const InitProblemDev* problems;
  const double* columns;          // per problem: u_ref[n], v_ref[n], u_cur[n], v_cur[n]
  svoh_homography_result* results;
  uint8_t* masks;
  int32_t n_hypotheses;
  int32_t lds_matches;            // capacity of the LDS columns (even, >= every n of the launch)
};

__device__ __forceinline__ unsigned long long init_mix(unsigned long long x)
{
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// r mod n for n <= 1024 in 32-bit arithmetic: r = hi 2^32 + lo, and (hi mod n)(2^32 mod n) + (lo mod n) < 2^21
__device__ __forceinline__ unsigned init_mod(unsigned long long r, unsigned n, unsigned two32_mod_n)
{
  const unsigned hi = (unsigned)(r >> 32), lo = (unsigned)r;
  return ((hi % n) * two32_mod_n + lo % n) % n;
}

// the matrix [l1 p1, l2 p2, l3 p3] that sends the projective basis to p1..p4 (third coordinates 1); its last row is lambda
__device__ __forceinline__ void init_basis(const double (&x)[4], const double (&y)[4], double (&M)[9])
{
  // p2 x p3, p3 x p1, p1 x p2, each dotted with p4
  const double l1 = (y[1] - y[2]) * x[3] + (x[2] - x[1]) * y[3] + (x[1] * y[2] - y[1] * x[2]);
  const double l2 = (y[2] - y[0]) * x[3] + (x[0] - x[2]) * y[3] + (x[2] * y[0] - y[2] * x[0]);
  const double l3 = (y[0] - y[1]) * x[3] + (x[1] - x[0]) * y[3] + (x[0] * y[1] - y[0] * x[1]);
  // column-wise: M = [l1 p1, l2 p2, l3 p3], stored row-major
  M[0] = l1 * x[0]; M[1] = l2 * x[1]; M[2] = l3 * x[2];
  M[3] = l1 * y[0]; M[4] = l2 * y[1]; M[5] = l3 * y[2];
  M[6] = l1;        M[7] = l2;        M[8] = l3;
}

__device__ __forceinline__ bool init_lambda_ok(const double (&M)[9])
{
  return fabs(M[6]) >= 1e-9 && fabs(M[7]) >= 1e-9 && fabs(M[8]) >= 1e-9;   // false for a NaN
}

__device__ __forceinline__ bool init_is_inlier(const double (&H)[9], double ur, double vr, double uc, double vc, double thresh2)
{
  const double x = H[0] * ur + H[1] * vr + H[2];
  const double y = H[3] * ur + H[4] * vr + H[5];
  const double w = H[6] * ur + H[7] * vr + H[8];
  const double dx = x - uc * w, dy = y - vc * w;
  return dx * dx + dy * dy < thresh2 * (w * w);   // false for w == 0 and for a NaN
}

__device__ __forceinline__ bool init_finite(double v) { return fabs(v) <= DBL_MAX; }

}  // namespace

__global__ __launch_bounds__(kInitThreads) void homography_ransac_kernel(const InitArgs a)
{
  extern __shared__ __attribute__((aligned(16))) double s_cols[];   // 4 x lds_matches (even: every column 16-byte aligned)
  __shared__ unsigned long long s_key[kInitWaves];
  __shared__ double s_H[9];
  __shared__ double s_red[kInitWaves][kInitNAcc];
  __shared__ int s_cnt[kInitWaves];
  __shared__ int s_stop, s_iters;

  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const InitProblemDev pb = a.problems[blockIdx.x];
  const int n = pb.n;
  const int cap = a.lds_matches;
  double* s_ur = s_cols;
  double* s_vr = s_cols + cap;
  double* s_uc = s_cols + 2 * cap;
  double* s_vc = s_cols + 3 * cap;
  svoh_homography_result* res = a.results + blockIdx.x;
  uint8_t* mask = a.masks + pb.first;

  {
    const double* g = a.columns + 4 * (size_t)pb.first;
    for (int i = tid; i < n; i += kInitThreads) {
      s_ur[i] = g[i]; s_vr[i] = g[n + i]; s_uc[i] = g[2 * n + i]; s_vc[i] = g[3 * n + i];
    }
  }
  __syncthreads();
  const double thresh2 = pb.thresh * pb.thresh;

  // ---- hypotheses: thread t takes t, t + 256, ... ----
  unsigned long long best_key = 0;   // (count + 1) << 32 | ~h: larger count first, then lower h; 0 = no model
  double bestH[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
  if (n >= 4) {
    const unsigned un = (unsigned)n;
    const unsigned two32_mod_n = (unsigned)(0x100000000ull % un);
    for (int h = tid; h < a.n_hypotheses; h += kInitThreads) {
      unsigned i0 = 0, i1 = 0, i2 = 0, i3 = 0;
      int kept = 0;
      for (int d = 0; d < kInitMaxDraws && kept < 4; ++d) {
        const unsigned long long r = init_mix(pb.seed ^ init_mix(((unsigned long long)(unsigned)h << 8) + (unsigned long long)d));
        const unsigned idx = init_mod(r, un, two32_mod_n);
        const bool seen = (kept > 0 && idx == i0) || (kept > 1 && idx == i1) || (kept > 2 && idx == i2);
        if (!seen) {
          if (kept == 0) i0 = idx; else if (kept == 1) i1 = idx; else if (kept == 2) i2 = idx; else i3 = idx;
          ++kept;
        }
      }
      if (kept < 4) continue;
      double A[9], B[9], H[9];
      {
        const double x[4] = { s_ur[i0], s_ur[i1], s_ur[i2], s_ur[i3] }, y[4] = { s_vr[i0], s_vr[i1], s_vr[i2], s_vr[i3] };
        init_basis(x, y, A);
      }
      {
        const double x[4] = { s_uc[i0], s_uc[i1], s_uc[i2], s_uc[i3] }, y[4] = { s_vc[i0], s_vc[i1], s_vc[i2], s_vc[i3] };
        init_basis(x, y, B);
      }
      if (!(init_lambda_ok(A) && init_lambda_ok(B))) continue;
      {
        // adj(A): rows a2 x a3, a3 x a1, a1 x a2 over A's columns a1, a2, a3
        double J[9];
        J[0] = A[4] * A[8] - A[7] * A[5]; J[1] = A[7] * A[2] - A[1] * A[8]; J[2] = A[1] * A[5] - A[4] * A[2];
        J[3] = A[5] * A[6] - A[8] * A[3]; J[4] = A[8] * A[0] - A[2] * A[6]; J[5] = A[2] * A[3] - A[5] * A[0];
        J[6] = A[3] * A[7] - A[6] * A[4]; J[7] = A[6] * A[1] - A[0] * A[7]; J[8] = A[0] * A[4] - A[3] * A[1];
        double s = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const double v = B[3 * r] * J[c] + B[3 * r + 1] * J[3 + c] + B[3 * r + 2] * J[6 + c];
            H[3 * r + c] = v;
            s += v * v;
          }
        const double norm = sqrt(s);
        if (!(norm > 0.0 && init_finite(norm))) continue;
#pragma unroll
        for (int k = 0; k < 9; ++k) H[k] /= norm;
      }
      int count = 0;
      for (int i = 0; i < n; ++i)   // the same address for all lanes: an LDS broadcast
        count += init_is_inlier(H, s_ur[i], s_vr[i], s_uc[i], s_vc[i], thresh2) ? 1 : 0;
      const unsigned long long key = ((unsigned long long)(unsigned)(count + 1) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)h);
      if (key > best_key) {
        best_key = key;
#pragma unroll
        for (int k = 0; k < 9; ++k) bestH[k] = H[k];
      }
    }
  }

  // ---- argmax over (count, lowest h): inside the wave, then over the four waves through LDS ----
  unsigned long long wkey = best_key;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long o = __shfl_xor(wkey, off, 64);
    wkey = o > wkey ? o : wkey;
  }
  if (lane == 0) s_key[wave] = wkey;
  __syncthreads();
  unsigned long long gkey = s_key[0];
#pragma unroll
  for (int w = 1; w < kInitWaves; ++w) gkey = s_key[w] > gkey ? s_key[w] : gkey;
  const int best_count = (int)(unsigned)(gkey >> 32) - 1;
  const int best_h = (int)(0xFFFFFFFFu - (unsigned)gkey);
  if (gkey == 0 || best_count < 4) {   // SVOH_HOMOGRAPHY_NO_MODEL: every output zero
    if (tid == 0) {
      for (int k = 0; k < 9; ++k) res->H[k] = 0.0;
      res->best_hypothesis = 0; res->n_inliers_hypothesis = 0; res->n_inliers = 0; res->refine_iters = 0;
      res->status = SVOH_HOMOGRAPHY_NO_MODEL; res->reserved = 0;
    }
    for (int i = tid; i < n; i += kInitThreads) mask[i] = 0;
    return;
  }
  if (best_key == gkey) {   // keys are unique: h is part of them
#pragma unroll
    for (int k = 0; k < 9; ++k) s_H[k] = bestH[k];
  }
  __syncthreads();

  // ---- refinement on the winner's inliers ----
  double H0[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) H0[k] = s_H[k];
  unsigned mine = 0;   // bit k: match tid + 256 k is an inlier of the winning hypothesis
#pragma unroll
  for (int k = 0; k < kInitMaxMatches / kInitThreads; ++k) {
    const int i = tid + k * kInitThreads;
    if (i < n && init_is_inlier(H0, s_ur[i], s_vr[i], s_uc[i], s_vc[i], thresh2)) mine |= 1u << k;
  }
  const bool refine = fabs(H0[8]) >= 1e-12;
  __syncthreads();   // every thread has read the hypothesis before it is scaled
  if (tid == 0) {
    if (refine) {
      const double h8 = s_H[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) s_H[k] /= h8;
      s_H[8] = 1.0;
    }
    s_stop = refine ? 0 : 1;
    s_iters = 0;
  }
  __syncthreads();
  for (int iter = 0; iter < kInitMaxRefineIters; ++iter) {
    if (s_stop) break;   // the same word for every thread, written before the barrier below
    double H[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) H[k] = s_H[k];
    double acc[kInitNAcc];
#pragma unroll
    for (int k = 0; k < kInitNAcc; ++k) acc[k] = 0.0;
#pragma unroll
    for (int k = 0; k < kInitMaxMatches / kInitThreads; ++k) {
      if (mine & (1u << k)) {
        const int i = tid + k * kInitThreads;
        const double u = s_ur[i], v = s_vr[i];
        const double x = H[0] * u + H[1] * v + H[2];
        const double y = H[3] * u + H[4] * v + H[5];
        const double w = H[6] * u + H[7] * v + H[8];
        const double iw = 1.0 / w;
        const double px = x * iw, py = y * iw;
        const double rx = px - s_uc[i], ry = py - s_vc[i];
        const double Jx[8] = { u * iw, v * iw, iw, 0.0, 0.0, 0.0, -px * u * iw, -px * v * iw };
        const double Jy[8] = { 0.0, 0.0, 0.0, u * iw, v * iw, iw, -py * u * iw, -py * v * iw };
#pragma unroll
        for (int r = 0; r < 8; ++r) {
#pragma unroll
          for (int c = 0; c <= r; ++c) acc[r * (r + 1) / 2 + c] += Jx[r] * Jx[c] + Jy[r] * Jy[c];
          acc[36 + r] -= Jx[r] * rx + Jy[r] * ry;
        }
      }
    }
    {
      int ridx;
      bool rvalid;
      wave_reduce_scatter<kInitNAcc>(acc, lane, ridx, rvalid);
      if (rvalid) s_red[wave][ridx] = acc[0];
    }
    __syncthreads();
    if (tid == 0) {
      double m[36], dx[8];
#pragma unroll
      for (int k = 0; k < 36; ++k) m[k] = (s_red[0][k] + s_red[1][k]) + (s_red[2][k] + s_red[3][k]);
#pragma unroll
      for (int k = 0; k < 8; ++k) dx[k] = (s_red[0][36 + k] + s_red[1][36 + k]) + (s_red[2][36 + k] + s_red[3][36 + k]);
      ldlt_solve_regs<8>(m, dx);
      bool finite = true;
      double biggest = 0.0;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        finite = finite && init_finite(dx[k]);
        biggest = fmax(biggest, fabs(dx[k]));
      }
      s_iters = iter + 1;
      if (!finite) s_stop = 1;   // the previous H stays
      else {
#pragma unroll
        for (int k = 0; k < 8; ++k) s_H[k] += dx[k];
        if (biggest < 1e-10) s_stop = 1;
      }
    }
    __syncthreads();
  }

  // ---- final mask and count (homography.cpp:47-56) with the refined H ----
  double H[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) H[k] = s_H[k];
  int count = 0;
#pragma unroll
  for (int k = 0; k < kInitMaxMatches / kInitThreads; ++k) {
    const int i = tid + k * kInitThreads;
    if (i < n) {
      const bool in = init_is_inlier(H, s_ur[i], s_vr[i], s_uc[i], s_vc[i], thresh2);
      mask[i] = in ? 1 : 0;
      count += in ? 1 : 0;
    }
  }
  count = wave_sum_i32_dpp(count);
  if (lane == 0) s_cnt[wave] = count;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) res->H[k] = H[k];
    res->best_hypothesis = best_h;
    res->n_inliers_hypothesis = best_count;
    res->n_inliers = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
    res->refine_iters = s_iters;
    res->status = SVOH_HOMOGRAPHY_OK;
    res->reserved = 0;
  }
}

// ---- the translation estimator (include/svo_hip.h, svoh_translation_ransac_batch) ----------------------------------------
// The reference's TwoPointInit runs OpenGV's RANSAC over TranslationSacProblemWithTriangulation (initialization.cpp:167-289);
// its sampling and early stop are OpenGV's, so the estimator is our own and deterministic, with the reference's score:
//   1. a match is staged as f_cur, g = R_cur_ref f_ref and the inverse of its 2x2 triangulation matrix (nine columns in LDS);
//   2. hypothesis h draws two different matches from the counter-based generator;
//   3. t = m_i x m_j, m = f_cur x g, normalised, pointing from where the ray was to where it is;
//   4. every hypothesis is scored on every match (translation_count_inliers: a model in, its count out);
//   5. the winner's inliers give M = sum mhat mhat^T, the refined t is the eigenvector of its smallest eigenvalue;
//   6. the mask and the count with the refined t.
// The per-hypothesis maths is svoh_translation.h's, shared with the host.
namespace {

struct TranslationProblemDev {
  double R[9];
  double thresh;
  unsigned long long seed;
  int32_t n;
  int32_t first;        // the problem's first match in the mask array; its bearings start at double 6 * first
};

struct TranslationArgs {
  const TranslationProblemDev* problems;
  const double* bearings;         // per problem: f_cur[3 n], f_ref[3 n]
  svoh_translation_result* results;
  uint8_t* masks;
  int32_t n_hypotheses;
  int32_t lds_matches;            // capacity of the LDS columns (even, >= every n of the launch)
};

}  // namespace

__global__ __launch_bounds__(kInitThreads) void translation_ransac_kernel(const TranslationArgs a)
{
  extern __shared__ __attribute__((aligned(16))) double s_cols[];   // kTranslationCols x lds_matches
  __shared__ unsigned long long s_key[kInitWaves];
  __shared__ double s_t[3];
  __shared__ double s_red[kInitWaves][6];
  __shared__ int s_cnt[kInitWaves], s_deg[kInitWaves];

  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const TranslationProblemDev* pb = a.problems + blockIdx.x;
  const int n = pb->n;
  const int cap = a.lds_matches;
  const double thresh = pb->thresh;
  const unsigned long long seed = pb->seed;
  svoh_translation_result* res = a.results + blockIdx.x;
  uint8_t* mask = a.masks + pb->first;

  {
    double R[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = pb->R[k];
    const double* fc = a.bearings + 6 * (size_t)pb->first;
    const double* fr = fc + 3 * (size_t)n;
    for (int i = tid; i < n; i += kInitThreads) {
      const double f_cur[3] = { fc[3 * i], fc[3 * i + 1], fc[3 * i + 2] }, f_ref[3] = { fr[3 * i], fr[3 * i + 1], fr[3 * i + 2] };
      double col[kTranslationCols];
      translation_stage(R, f_cur, f_ref, col);
#pragma unroll
      for (int k = 0; k < kTranslationCols; ++k) s_cols[k * cap + i] = col[k];
    }
  }
  __syncthreads();

  // ---- hypotheses: thread t takes t, t + 256, ... ----
  unsigned long long best_key = 0;   // (count + 1) << 32 | ~h: larger count first, then lower h; 0 = no model
  double best_t[3] = { 0, 0, 0 };
  int n_degenerate = 0;
  if (n >= 2) {
    for (int h = tid; h < a.n_hypotheses; h += kInitThreads) {
      unsigned i, j;
      double t[3];
      bool ok = translation_sample(seed, (unsigned)h, (unsigned)n, i, j);
      if (ok) {
        const double fi[3] = { s_cols[i], s_cols[cap + i], s_cols[2 * cap + i] }, gi[3] = { s_cols[3 * cap + i], s_cols[4 * cap + i], s_cols[5 * cap + i] };
        const double fj[3] = { s_cols[j], s_cols[cap + j], s_cols[2 * cap + j] }, gj[3] = { s_cols[3 * cap + j], s_cols[4 * cap + j], s_cols[5 * cap + j] };
        ok = translation_from_two(fi, gi, fj, gj, t);
      }
      if (!ok) { ++n_degenerate; continue; }
      const int count = translation_count_inliers(t, s_cols, cap, n, thresh);   // the same address for all lanes: an LDS broadcast
      const unsigned long long key = ((unsigned long long)(unsigned)(count + 1) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)h);
      if (key > best_key) {
        best_key = key;
        best_t[0] = t[0]; best_t[1] = t[1]; best_t[2] = t[2];
      }
    }
  }

  // ---- argmax over (count, lowest h) and the number of degenerate hypotheses ----
  unsigned long long wkey = best_key;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long o = __shfl_xor(wkey, off, 64);
    wkey = o > wkey ? o : wkey;
  }
  n_degenerate = wave_sum_i32_dpp(n_degenerate);
  if (lane == 0) { s_key[wave] = wkey; s_deg[wave] = n_degenerate; }
  __syncthreads();
  unsigned long long gkey = s_key[0];
#pragma unroll
  for (int w = 1; w < kInitWaves; ++w) gkey = s_key[w] > gkey ? s_key[w] : gkey;
  const int best_count = (int)(unsigned)(gkey >> 32) - 1;
  const int best_h = (int)(0xFFFFFFFFu - (unsigned)gkey);
  if (gkey == 0 || best_count < 2) {   // SVOH_TRANSLATION_NO_MODEL: every output zero
    if (tid == 0) {
      res->t[0] = res->t[1] = res->t[2] = 0.0;
      res->best_hypothesis = 0; res->n_inliers_hypothesis = 0; res->n_inliers = 0; res->n_degenerate = 0;
      res->status = SVOH_TRANSLATION_NO_MODEL; res->reserved = 0;
    }
    for (int i = tid; i < n; i += kInitThreads) mask[i] = 0;
    return;
  }
  if (best_key == gkey) {   // keys are unique: h is part of them
    s_t[0] = best_t[0]; s_t[1] = best_t[1]; s_t[2] = best_t[2];
  }
  __syncthreads();

  // ---- refinement on the winner's inliers ----
  const double t0[3] = { s_t[0], s_t[1], s_t[2] };
  double acc[6] = { 0, 0, 0, 0, 0, 0 };
#pragma unroll
  for (int k = 0; k < kInitMaxMatches / kInitThreads; ++k) {
    const int i = tid + k * kInitThreads;
    if (i < n && translation_is_inlier(t0, s_cols, cap, i, thresh)) translation_accumulate(s_cols, cap, i, acc);
  }
  {
    int ridx;
    bool rvalid;
    wave_reduce_scatter<6>(acc, lane, ridx, rvalid);
    if (rvalid) s_red[wave][ridx] = acc[0];
  }
  __syncthreads();   // (every thread has read the winner's t before it is replaced)
  if (tid == 0) {
    double M[6], t[3];
#pragma unroll
    for (int k = 0; k < 6; ++k) M[k] = (s_red[0][k] + s_red[1][k]) + (s_red[2][k] + s_red[3][k]);
    translation_refine(M, t0, t);
    s_t[0] = t[0]; s_t[1] = t[1]; s_t[2] = t[2];
  }
  __syncthreads();

  // ---- final mask and count with the refined t ----
  const double t[3] = { s_t[0], s_t[1], s_t[2] };
  int count = 0;
#pragma unroll
  for (int k = 0; k < kInitMaxMatches / kInitThreads; ++k) {
    const int i = tid + k * kInitThreads;
    if (i < n) {
      const bool in = translation_is_inlier(t, s_cols, cap, i, thresh);
      mask[i] = in ? 1 : 0;
      count += in ? 1 : 0;
    }
  }
  count = wave_sum_i32_dpp(count);
  if (lane == 0) s_cnt[wave] = count;
  __syncthreads();
  if (tid == 0) {
    res->t[0] = t[0]; res->t[1] = t[1]; res->t[2] = t[2];
    res->best_hypothesis = best_h;
    res->n_inliers_hypothesis = best_count;
    res->n_inliers = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
    res->n_degenerate = (s_deg[0] + s_deg[1]) + (s_deg[2] + s_deg[3]);
    res->status = SVOH_TRANSLATION_OK;
    res->reserved = 0;
  }
}

}  // namespace svoh

using namespace svoh;

extern "C" int svoh_homography_ransac_batch(svoh_ctx* ctx, const svoh_init_options* options, int n_problems,
                                            const svoh_homography_problem* problems, svoh_homography_result* results, uint8_t* masks)
try {
  if (!ctx) return set_error(nullptr, SVOH_ERR_INVALID_ARGUMENT, "ctx is NULL");
  SVOH_REQUIRE(ctx, options != nullptr, "NULL argument");
  SVOH_REQUIRE(ctx, n_problems >= 0, "negative count");
  SVOH_REQUIRE(ctx, options->n_hypotheses >= 0 && options->n_hypotheses <= (1 << 24), "n_hypotheses out of range (0 .. 2^24)");
  if (n_problems == 0) return SVOH_OK;
  SVOH_REQUIRE(ctx, problems && results, "NULL argument");
  size_t total = 0;
  int max_n = 0;
  for (int p = 0; p < n_problems; ++p) {
    const svoh_homography_problem& pb = problems[p];
    SVOH_REQUIRE(ctx, pb.n >= 0 && pb.n <= kInitMaxMatches, "a homography problem has more than 1024 matches (or a negative count)");
    SVOH_REQUIRE(ctx, pb.n == 0 || (pb.uv_ref && pb.uv_cur), "NULL match array");
    total += (size_t)pb.n;
    max_n = std::max(max_n, pb.n);
  }
  SVOH_REQUIRE(ctx, total == 0 || masks, "NULL mask array");
  SVOH_REQUIRE(ctx, total <= (size_t)1 << 30, "too many matches in one call");
  SVOH_HIP_TRY(ctx, hipSetDevice(ctx->device));
  SVOH_ALIGN_JOIN(ctx);
  auto al = [](size_t x) { return (x + 63) & ~(size_t)63; };
  const size_t o_pb = 0, o_cols = al(sizeof(InitProblemDev) * (size_t)n_problems);
  const size_t o_res = o_cols + al(32 * (total ? total : 1));
  const size_t o_mask = o_res + al(sizeof(svoh_homography_result) * (size_t)n_problems);
  const size_t bytes = o_mask + al(total ? total : 1);
  SVOH_HIP_TRY(ctx, ctx->h_scratch0.reserve(bytes));
  SVOH_HIP_TRY(ctx, ctx->d_scratch0.reserve(bytes));
  uint8_t* h = static_cast<uint8_t*>(ctx->h_scratch0.ptr);
  uint8_t* d = static_cast<uint8_t*>(ctx->d_scratch0.ptr);
  InitProblemDev* hp = reinterpret_cast<InitProblemDev*>(h + o_pb);
  double* hc = reinterpret_cast<double*>(h + o_cols);
  size_t first = 0;
  for (int p = 0; p < n_problems; ++p) {
    const svoh_homography_problem& pb = problems[p];
    hp[p].thresh = pb.thresh; hp[p].seed = pb.seed; hp[p].n = pb.n; hp[p].first = (int32_t)first; hp[p].pad_[0] = hp[p].pad_[1] = 0;
    double* c = hc + 4 * first;
    const size_t n = (size_t)pb.n;
    for (size_t i = 0; i < n; ++i) {
      c[i] = pb.uv_ref[2 * i]; c[n + i] = pb.uv_ref[2 * i + 1];
      c[2 * n + i] = pb.uv_cur[2 * i]; c[3 * n + i] = pb.uv_cur[2 * i + 1];
    }
    first += n;
  }
  SVOH_HIP_TRY(ctx, svoh_copy_to_device(ctx, d, h, o_res));
  InitArgs a;
  a.problems = reinterpret_cast<const InitProblemDev*>(d + o_pb);
  a.columns = reinterpret_cast<const double*>(d + o_cols);
  a.results = reinterpret_cast<svoh_homography_result*>(d + o_res);
  a.masks = d + o_mask;
  a.n_hypotheses = options->n_hypotheses;
  a.lds_matches = std::max(2, (max_n + 1) & ~1);
  const size_t lds = 4 * sizeof(double) * (size_t)a.lds_matches;
  hipStream_t stream = ctx->stream;
  const bool timed = ctx->timing_on();
  if (timed) SVOH_HIP_TRY(ctx, hipEventRecord(ctx->ev_misc_start, stream));
  hipLaunchKernelGGL(homography_ransac_kernel, dim3((unsigned)n_problems), dim3(kInitThreads), lds, stream, a);
  SVOH_HIP_TRY(ctx, hipGetLastError());
  if (timed) SVOH_HIP_TRY(ctx, hipEventRecord(ctx->ev_misc_stop, stream));
  ctx->misc_timed = timed; ctx->misc_launched = true;
  SVOH_HIP_TRY(ctx, svoh_copy_to_host(ctx, h + o_res, d + o_res, bytes - o_res));
  SVOH_HIP_TRY(ctx, hipStreamSynchronize(stream));
  memcpy(results, h + o_res, sizeof(svoh_homography_result) * (size_t)n_problems);
  if (total) memcpy(masks, h + o_mask, total);
  return SVOH_OK;
} SVOH_ABI_CATCH(ctx)

extern "C" int svoh_translation_ransac_batch(svoh_ctx* ctx, const svoh_init_options* options, int n_problems,
                                             const svoh_translation_problem* problems, svoh_translation_result* results, uint8_t* masks)
try {
  if (!ctx) return set_error(nullptr, SVOH_ERR_INVALID_ARGUMENT, "ctx is NULL");
  SVOH_REQUIRE(ctx, options != nullptr, "NULL argument");
  SVOH_REQUIRE(ctx, n_problems >= 0, "negative count");
  SVOH_REQUIRE(ctx, options->n_hypotheses >= 0 && options->n_hypotheses <= (1 << 24), "n_hypotheses out of range (0 .. 2^24)");
  if (n_problems == 0) return SVOH_OK;
  SVOH_REQUIRE(ctx, problems && results, "NULL argument");
  size_t total = 0;
  int max_n = 0;
  for (int p = 0; p < n_problems; ++p) {
    const svoh_translation_problem& pb = problems[p];
    SVOH_REQUIRE(ctx, pb.n >= 0 && pb.n <= kInitMaxMatches, "a translation problem has more than 1024 matches (or a negative count)");
    SVOH_REQUIRE(ctx, pb.n == 0 || (pb.f_cur && pb.f_ref), "NULL bearing array");
    total += (size_t)pb.n;
    max_n = std::max(max_n, pb.n);
  }
  SVOH_REQUIRE(ctx, total == 0 || masks, "NULL mask array");
  SVOH_REQUIRE(ctx, total <= (size_t)1 << 30, "too many matches in one call");
  SVOH_HIP_TRY(ctx, hipSetDevice(ctx->device));
  SVOH_ALIGN_JOIN(ctx);
  auto al = [](size_t x) { return (x + 63) & ~(size_t)63; };
  const size_t o_pb = 0, o_f = al(sizeof(TranslationProblemDev) * (size_t)n_problems);
  const size_t o_res = o_f + al(48 * (total ? total : 1));
  const size_t o_mask = o_res + al(sizeof(svoh_translation_result) * (size_t)n_problems);
  const size_t bytes = o_mask + al(total ? total : 1);
  SVOH_HIP_TRY(ctx, ctx->h_scratch0.reserve(bytes));
  SVOH_HIP_TRY(ctx, ctx->d_scratch0.reserve(bytes));
  uint8_t* h = static_cast<uint8_t*>(ctx->h_scratch0.ptr);
  uint8_t* d = static_cast<uint8_t*>(ctx->d_scratch0.ptr);
  TranslationProblemDev* hp = reinterpret_cast<TranslationProblemDev*>(h + o_pb);
  double* hf = reinterpret_cast<double*>(h + o_f);
  size_t first = 0;
  for (int p = 0; p < n_problems; ++p) {
    const svoh_translation_problem& pb = problems[p];
    memcpy(hp[p].R, pb.R_cur_ref, sizeof hp[p].R);
    hp[p].thresh = pb.thresh; hp[p].seed = pb.seed; hp[p].n = pb.n; hp[p].first = (int32_t)first;
    const size_t n = (size_t)pb.n;
    if (n) {
      memcpy(hf + 6 * first, pb.f_cur, 3 * n * sizeof(double));
      memcpy(hf + 6 * first + 3 * n, pb.f_ref, 3 * n * sizeof(double));
    }
    first += n;
  }
  SVOH_HIP_TRY(ctx, svoh_copy_to_device(ctx, d, h, o_res));
  TranslationArgs a;
  a.problems = reinterpret_cast<const TranslationProblemDev*>(d + o_pb);
  a.bearings = reinterpret_cast<const double*>(d + o_f);
  a.results = reinterpret_cast<svoh_translation_result*>(d + o_res);
  a.masks = d + o_mask;
  a.n_hypotheses = options->n_hypotheses;
  a.lds_matches = std::max(2, (max_n + 1) & ~1);
  const size_t lds = kTranslationCols * sizeof(double) * (size_t)a.lds_matches;   // 72 KB at 1024 matches
  if (lds > 48 * 1024)
    SVOH_HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(translation_ransac_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipStream_t stream = ctx->stream;
  const bool timed = ctx->timing_on();
  if (timed) SVOH_HIP_TRY(ctx, hipEventRecord(ctx->ev_misc_start, stream));
  hipLaunchKernelGGL(translation_ransac_kernel, dim3((unsigned)n_problems), dim3(kInitThreads), lds, stream, a);
  SVOH_HIP_TRY(ctx, hipGetLastError());
  if (timed) SVOH_HIP_TRY(ctx, hipEventRecord(ctx->ev_misc_stop, stream));
  ctx->misc_timed = timed; ctx->misc_launched = true;
  SVOH_HIP_TRY(ctx, svoh_copy_to_host(ctx, h + o_res, d + o_res, bytes - o_res));
  SVOH_HIP_TRY(ctx, hipStreamSynchronize(stream));
  memcpy(results, h + o_res, sizeof(svoh_translation_result) * (size_t)n_problems);
  if (total) memcpy(masks, h + o_mask, total);
  return SVOH_OK;
} SVOH_ABI_CATCH(ctx)
