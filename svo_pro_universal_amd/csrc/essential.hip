// essential.hip -- the essential-matrix estimator of the mono bootstrap (include/svo_hip.h, svoh_essential_ransac_batch;
// DESIGN.md, "FivePoint initialiser"): a batch of RANSAC problems, one workgroup of 256 threads per problem, as the two
// estimators of init.hip.
//
// The reference's FivePointInit runs OpenGV's RANSAC over CentralRelativePoseSacProblem with Nister's solver
// (initialization.cpp:292-359); its sampling and early stop are OpenGV's, so the estimator is our own and a function of its
// inputs alone, with the score of the TwoPoint estimator:
//   1. hypothesis h draws five different matches from the counter-based generator;
//   2. the essential matrices of the five (svoh_essential.h: null space, ten cubics, elimination, degree-10 polynomial, its
//      real roots in ascending order), in per-thread local arrays;
//   3. of a candidate's four motions the first that holds the five;
//   4. every candidate is scored on every match (essential_count_inliers: a model in, its count out);
//   5. Gauss-Newton over (rotation, direction of t) on the winner's inliers, normal equations in fp64;
//   6. the mask and the count with the refined motion.
// The matches of a problem lie in LDS as six columns of doubles; in the scoring loop all lanes of a wave read the same match
// (one address: a broadcast), each lane with a motion of its own in registers.  No global atomics, nothing shared between
// workgroups, no waiting; every loop is bounded by n, K or a constant.
#include <cmath>
#include <cstring>
#include <vector>

#include "svoh_internal.h"
#include "svoh_device_utils.h"
#include "svoh_essential.h"

namespace svoh {

namespace {

constexpr int kEsThreads = 256;
constexpr int kEsWaves = kEsThreads / 64;
constexpr int kEsMaxMatches = 1024;   // 6 columns x 1024 x 8 bytes = 48 KB of LDS
constexpr int kEsMaxRefineIters = 10;

struct EssentialProblemDev {
  double thresh;
  unsigned long long seed;
  int32_t n;
  int32_t first;        // the problem's first match in the mask array; its bearings start at double 6 * first
};

struct EssentialArgs {
  const EssentialProblemDev* problems;
  const double* bearings;         // per problem: f_cur[3 n], f_ref[3 n]
  svoh_essential_result* results;
  uint8_t* masks;
  int32_t n_hypotheses;
  int32_t lds_matches;            // capacity of the LDS columns (even, >= every n of the launch)
};

}  // namespace

__global__ __launch_bounds__(kEsThreads) void essential_ransac_kernel(const EssentialArgs a)
{
  extern __shared__ __attribute__((aligned(16))) double s_cols[];   // kEssentialCols x lds_matches
  __shared__ unsigned long long s_key[kEsWaves];
  __shared__ double s_R[9], s_t[3];
  __shared__ double s_red[kEsWaves][kEssentialNAcc];
  __shared__ int s_cnt[kEsWaves], s_deg[kEsWaves], s_mod[kEsWaves];
  __shared__ int s_stop, s_iters;

  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const EssentialProblemDev* pb = a.problems + blockIdx.x;
  const int n = pb->n;
  const int cap = a.lds_matches;
  const double thresh = pb->thresh;
  const unsigned long long seed = pb->seed;
  svoh_essential_result* res = a.results + blockIdx.x;
  uint8_t* mask = a.masks + pb->first;

  {
    const double* fc = a.bearings + 6 * (size_t)pb->first;
    const double* fr = fc + 3 * (size_t)n;
    for (int i = tid; i < n; i += kEsThreads) {
#pragma unroll
      for (int k = 0; k < 3; ++k) { s_cols[k * cap + i] = fc[3 * i + k]; s_cols[(3 + k) * cap + i] = fr[3 * i + k]; }
    }
  }
  __syncthreads();

  // ---- hypotheses: thread t takes t, t + 256, ... ----
  unsigned long long best_key = 0;   // (count + 1) << 36 | ~h << 4 | ~candidate: larger count, lower h, lower candidate; 0 = no model
  double best_R[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 }, best_t[3] = { 0, 0, 0 };
  int n_degenerate = 0, n_models = 0;
  if (n >= 5) {
#pragma unroll 1
    for (int h = tid; h < a.n_hypotheses; h += kEsThreads) {
      int models, count, candidate;
      double R[9], t[3];
      if (!essential_hypothesis(seed, (unsigned)h, s_cols, cap, n, thresh, models, count, candidate, R, t)) { ++n_degenerate; continue; }
      n_models += models;
      if (models == 0) continue;
      const unsigned long long key = ((unsigned long long)(unsigned)(count + 1) << 36) | ((unsigned long long)(0xFFFFFFFFu - (unsigned)h) << 4) |
                                     (unsigned long long)(15u - (unsigned)candidate);
      if (key > best_key) {
        best_key = key;
#pragma unroll
        for (int k = 0; k < 9; ++k) best_R[k] = R[k];
        best_t[0] = t[0]; best_t[1] = t[1]; best_t[2] = t[2];
      }
    }
  }

  // ---- argmax over (count, lowest h, lowest candidate), the degenerate hypotheses and the candidates scored ----
  unsigned long long wkey = best_key;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long o = __shfl_xor(wkey, off, 64);
    wkey = o > wkey ? o : wkey;
  }
  n_degenerate = wave_sum_i32_dpp(n_degenerate);
  n_models = wave_sum_i32_dpp(n_models);
  if (lane == 0) { s_key[wave] = wkey; s_deg[wave] = n_degenerate; s_mod[wave] = n_models; }
  __syncthreads();
  unsigned long long gkey = s_key[0];
#pragma unroll
  for (int w = 1; w < kEsWaves; ++w) gkey = s_key[w] > gkey ? s_key[w] : gkey;
  const int best_count = (int)(unsigned)(gkey >> 36) - 1;
  const int best_h = (int)(0xFFFFFFFFu - (unsigned)(gkey >> 4));
  const int best_c = (int)(15u - (unsigned)(gkey & 15u));
  if (gkey == 0 || best_count < 5) {   // SVOH_ESSENTIAL_NO_MODEL: every output zero
    if (tid == 0) {
#pragma unroll
      for (int k = 0; k < 9; ++k) res->R[k] = 0.0;
      res->t[0] = res->t[1] = res->t[2] = 0.0;
      res->best_hypothesis = 0; res->best_candidate = 0; res->n_inliers_hypothesis = 0; res->n_inliers = 0;
      res->n_degenerate = 0; res->n_models = 0; res->refine_iters = 0; res->status = SVOH_ESSENTIAL_NO_MODEL;
      res->reserved[0] = res->reserved[1] = 0;
    }
    for (int i = tid; i < n; i += kEsThreads) mask[i] = 0;
    return;
  }
  if (best_key == gkey) {   // keys are unique: h and the candidate are part of them
#pragma unroll
    for (int k = 0; k < 9; ++k) s_R[k] = best_R[k];
    s_t[0] = best_t[0]; s_t[1] = best_t[1]; s_t[2] = best_t[2];
    s_stop = 0;
    s_iters = 0;
  }
  __syncthreads();

  // ---- refinement on the winner's inliers ----
  unsigned mine = 0;   // bit k: match tid + 256 k is an inlier of the winner
  {
    double R0[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) R0[k] = s_R[k];
    const double t0[3] = { s_t[0], s_t[1], s_t[2] };
#pragma unroll
    for (int k = 0; k < kEsMaxMatches / kEsThreads; ++k) {
      const int i = tid + k * kEsThreads;
      if (i < n && essential_is_inlier(R0, t0, s_cols, cap, i, thresh)) mine |= 1u << k;
    }
  }
#pragma unroll 1
  for (int iter = 0; iter < kEsMaxRefineIters; ++iter) {
    if (s_stop) break;   // the same word for every thread, written before the barrier below
    double R[9], b1[3], b2[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = s_R[k];
    const double t[3] = { s_t[0], s_t[1], s_t[2] };
    essential_tangent(t, b1, b2);
    double acc[kEssentialNAcc];
#pragma unroll
    for (int k = 0; k < kEssentialNAcc; ++k) acc[k] = 0.0;
#pragma unroll
    for (int k = 0; k < kEsMaxMatches / kEsThreads; ++k)
      if (mine & (1u << k)) essential_accumulate(R, t, b1, b2, s_cols, cap, tid + k * kEsThreads, acc);
    {
      int ridx;
      bool rvalid;
      wave_reduce_scatter<kEssentialNAcc>(acc, lane, ridx, rvalid);
      if (rvalid) s_red[wave][ridx] = acc[0];
    }
    __syncthreads();
    if (tid == 0) {
      double m[15], d[5];
#pragma unroll
      for (int k = 0; k < 15; ++k) m[k] = (s_red[0][k] + s_red[1][k]) + (s_red[2][k] + s_red[3][k]);
#pragma unroll
      for (int k = 0; k < 5; ++k) d[k] = (s_red[0][15 + k] + s_red[1][15 + k]) + (s_red[2][15 + k] + s_red[3][15 + k]);
      ldlt_solve_regs<5>(m, d);
      bool finite = true;
      double biggest = 0.0;
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        finite = finite && tr_finite(d[k]);
        biggest = fmax(biggest, fabs(d[k]));
      }
      s_iters = iter + 1;
      if (!finite) s_stop = 1;   // the previous motion stays
      else {
        double Rn[9], tn[3] = { t[0], t[1], t[2] };
#pragma unroll
        for (int k = 0; k < 9; ++k) Rn[k] = R[k];
        essential_update(d, b1, b2, Rn, tn);
#pragma unroll
        for (int k = 0; k < 9; ++k) s_R[k] = Rn[k];
        s_t[0] = tn[0]; s_t[1] = tn[1]; s_t[2] = tn[2];
        if (biggest < 1e-10) s_stop = 1;
      }
    }
    __syncthreads();
  }

  // ---- final mask and count with the refined motion ----
  double R[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = s_R[k];
  const double t[3] = { s_t[0], s_t[1], s_t[2] };
  int count = 0;
#pragma unroll
  for (int k = 0; k < kEsMaxMatches / kEsThreads; ++k) {
    const int i = tid + k * kEsThreads;
    if (i < n) {
      const bool in = essential_is_inlier(R, t, s_cols, cap, i, thresh);
      mask[i] = in ? 1 : 0;
      count += in ? 1 : 0;
    }
  }
  count = wave_sum_i32_dpp(count);
  if (lane == 0) s_cnt[wave] = count;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) res->R[k] = R[k];
    res->t[0] = t[0]; res->t[1] = t[1]; res->t[2] = t[2];
    res->best_hypothesis = best_h;
    res->best_candidate = best_c;
    res->n_inliers_hypothesis = best_count;
    res->n_inliers = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
    res->n_degenerate = (s_deg[0] + s_deg[1]) + (s_deg[2] + s_deg[3]);
    res->n_models = (s_mod[0] + s_mod[1]) + (s_mod[2] + s_mod[3]);
    res->refine_iters = s_iters;
    res->status = SVOH_ESSENTIAL_OK;
    res->reserved[0] = res->reserved[1] = 0;
  }
}

}  // namespace svoh

using namespace svoh;

extern "C" int svoh_essential_ransac_batch(svoh_ctx* ctx, const svoh_init_options* options, int n_problems,
                                           const svoh_essential_problem* problems, svoh_essential_result* results, uint8_t* masks)
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
    const svoh_essential_problem& pb = problems[p];
    SVOH_REQUIRE(ctx, pb.n >= 0 && pb.n <= kEsMaxMatches, "an essential-matrix problem has more than 1024 matches (or a negative count)");
    SVOH_REQUIRE(ctx, pb.n == 0 || (pb.f_cur && pb.f_ref), "NULL bearing array");
    total += (size_t)pb.n;
    max_n = std::max(max_n, pb.n);
  }
  SVOH_REQUIRE(ctx, total == 0 || masks, "NULL mask array");
  SVOH_REQUIRE(ctx, total <= (size_t)1 << 30, "too many matches in one call");
  SVOH_HIP_TRY(ctx, hipSetDevice(ctx->device));
  SVOH_ALIGN_JOIN(ctx);
  auto al = [](size_t x) { return (x + 63) & ~(size_t)63; };
  const size_t o_pb = 0, o_f = al(sizeof(EssentialProblemDev) * (size_t)n_problems);
  const size_t o_res = o_f + al(48 * (total ? total : 1));
  const size_t o_mask = o_res + al(sizeof(svoh_essential_result) * (size_t)n_problems);
  const size_t bytes = o_mask + al(total ? total : 1);
  SVOH_HIP_TRY(ctx, ctx->h_scratch0.reserve(bytes));
  SVOH_HIP_TRY(ctx, ctx->d_scratch0.reserve(bytes));
  uint8_t* h = static_cast<uint8_t*>(ctx->h_scratch0.ptr);
  uint8_t* d = static_cast<uint8_t*>(ctx->d_scratch0.ptr);
  EssentialProblemDev* hp = reinterpret_cast<EssentialProblemDev*>(h + o_pb);
  double* hf = reinterpret_cast<double*>(h + o_f);
  size_t first = 0;
  for (int p = 0; p < n_problems; ++p) {
    const svoh_essential_problem& pb = problems[p];
    hp[p].thresh = pb.thresh; hp[p].seed = pb.seed; hp[p].n = pb.n; hp[p].first = (int32_t)first;
    const size_t n = (size_t)pb.n;
    if (n) {
      memcpy(hf + 6 * first, pb.f_cur, 3 * n * sizeof(double));
      memcpy(hf + 6 * first + 3 * n, pb.f_ref, 3 * n * sizeof(double));
    }
    first += n;
  }
  SVOH_HIP_TRY(ctx, svoh_copy_to_device(ctx, d, h, o_res));
  EssentialArgs a;
  a.problems = reinterpret_cast<const EssentialProblemDev*>(d + o_pb);
  a.bearings = reinterpret_cast<const double*>(d + o_f);
  a.results = reinterpret_cast<svoh_essential_result*>(d + o_res);
  a.masks = d + o_mask;
  a.n_hypotheses = options->n_hypotheses;
  a.lds_matches = std::max(2, (max_n + 1) & ~1);
  const size_t lds = kEssentialCols * sizeof(double) * (size_t)a.lds_matches;   // 48 KB at 1024 matches
  if (lds > 40 * 1024)   // with the kernel's static words the sum may pass the 48 KB a launch gets unasked
    SVOH_HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(essential_ransac_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipStream_t stream = ctx->stream;
  const bool timed = ctx->timing_on();
  if (timed) SVOH_HIP_TRY(ctx, hipEventRecord(ctx->ev_misc_start, stream));
  hipLaunchKernelGGL(essential_ransac_kernel, dim3((unsigned)n_problems), dim3(kEsThreads), lds, stream, a);
  SVOH_HIP_TRY(ctx, hipGetLastError());
  if (timed) SVOH_HIP_TRY(ctx, hipEventRecord(ctx->ev_misc_stop, stream));
  ctx->misc_timed = timed; ctx->misc_launched = true;
  SVOH_HIP_TRY(ctx, svoh_copy_to_host(ctx, h + o_res, d + o_res, bytes - o_res));
  SVOH_HIP_TRY(ctx, hipStreamSynchronize(stream));
  memcpy(results, h + o_res, sizeof(svoh_essential_result) * (size_t)n_problems);
  if (total) memcpy(masks, h + o_mask, total);
  return SVOH_OK;
} SVOH_ABI_CATCH(ctx)
