// svo_hip_init.cpp -- the mono bootstrap's host side (see svo_hip_init.h).  The first part is plain maths (no device
// call; -DSVOH_INIT_MATH_ONLY stops there), the second part runs the estimator on the device and mirrors HomographyInit.
#include "svo_hip_init.h"

#include <algorithm>
#include <cmath>
#include <functional>
#include <limits>
#include <stdexcept>
#include <string>
#include <unordered_map>

namespace svo_hip {

namespace {
inline double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
inline double norm3(const double* a) { return std::sqrt(dot3(a, a)); }
inline void matvec3(const double M[9], const double v[3], double out[3])
{
  for (int r = 0; r < 3; ++r) out[r] = M[3 * r] * v[0] + M[3 * r + 1] * v[1] + M[3 * r + 2] * v[2];
}
inline void matTvec3(const double M[9], const double v[3], double out[3])
{
  for (int c = 0; c < 3; ++c) out[c] = M[c] * v[0] + M[3 + c] * v[1] + M[6 + c] * v[2];
}
inline void matmul3(const double A[9], const double B[9], double C[9])
{
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}
inline int signd(double x) { return x >= 0 ? 1 : -1; }   // homography_decomp.h:65-68
// HomographyDecompInria::oppositeOfMinor
inline double oppositeOfMinor(const double M[9], int row, int col)
{
  const int x1 = col == 0 ? 1 : 0, x2 = col == 2 ? 1 : 2, y1 = row == 0 ? 1 : 0, y2 = row == 2 ? 1 : 2;
  return M[3 * y1 + x2] * M[3 * y2 + x1] - M[3 * y1 + x1] * M[3 * y2 + x2];
}
// R = Hnorm (I - (2 / v) tstar n^T)
inline void findRmatFrom_tstar_n(const double Hn[9], const double tstar[3], const double n[3], double v, double R[9])
{
  double M[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) M[3 * r + c] = (r == c ? 1.0 : 0.0) - (2 / v) * tstar[r] * n[c];
  matmul3(Hn, M, R);
}
}  // namespace

namespace vk {

void singularValues3(const double H[9], double sv[3])
{
  // A = H^T H (symmetric), cyclic Jacobi: every rotation zeroes one off-diagonal pair
  double A[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) A[r][c] = H[r] * H[c] + H[3 + r] * H[3 + c] + H[6 + r] * H[6 + c];
  for (int sweep = 0; sweep < 30; ++sweep) {
    const double off = std::fabs(A[0][1]) + std::fabs(A[0][2]) + std::fabs(A[1][2]);
    const double diag = std::fabs(A[0][0]) + std::fabs(A[1][1]) + std::fabs(A[2][2]);
    if (!(off > 1e-30 * diag)) break;   // also ends on a NaN
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        if (A[p][q] == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 3; ++k) {   // A <- A J
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 3; ++k) {   // A <- J^T A
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk;
        }
      }
  }
  double e[3] = { A[0][0], A[1][1], A[2][2] };
  std::sort(e, e + 3, std::greater<double>());
  for (int i = 0; i < 3; ++i) sv[i] = std::sqrt(e[i] > 0.0 ? e[i] : 0.0);
}

void decomposeHomography(const double H[9], std::vector<CameraMotion>* motions)
{
  motions->clear();
  double sv[3];
  singularValues3(H, sv);
  double Hn[9];
  for (int i = 0; i < 9; ++i) Hn[i] = H[i] * (1.0 / sv[1]);   // removeScale
  const double epsilon = 0.001;
  double S[9];   // S = H'H - I
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) S[3 * r + c] = Hn[r] * Hn[c] + Hn[3 + r] * Hn[3 + c] + Hn[6 + r] * Hn[6 + c] - (r == c ? 1.0 : 0.0);
  double ninf = 0.0;   // norm(S, NORM_INF): the largest absolute row sum
  for (int r = 0; r < 3; ++r) ninf = std::max(ninf, std::fabs(S[3 * r]) + std::fabs(S[3 * r + 1]) + std::fabs(S[3 * r + 2]));
  if (ninf < epsilon) {   // H is a rotation
    CameraMotion m{};
    for (int i = 0; i < 9; ++i) m.R[i] = Hn[i];
    motions->push_back(m);
    return;
  }
  const double M00 = oppositeOfMinor(S, 0, 0), M11 = oppositeOfMinor(S, 1, 1), M22 = oppositeOfMinor(S, 2, 2);
  const double rtM00 = std::sqrt(M00), rtM11 = std::sqrt(M11), rtM22 = std::sqrt(M22);
  const double M01 = oppositeOfMinor(S, 0, 1), M12 = oppositeOfMinor(S, 1, 2), M02 = oppositeOfMinor(S, 0, 2);
  const int e12 = signd(M12), e02 = signd(M02), e01 = signd(M01);
  const double nS00 = std::fabs(S[0]), nS11 = std::fabs(S[4]), nS22 = std::fabs(S[8]);
  int indx = 0;   // max |Sii|
  if (nS00 < nS11) { indx = 1; if (nS11 < nS22) indx = 2; }
  else if (nS00 < nS22) indx = 2;
  double npa[3], npb[3];
  switch (indx) {
    case 0:
      npa[0] = S[0]; npb[0] = S[0];
      npa[1] = S[1] + rtM22; npb[1] = S[1] - rtM22;
      npa[2] = S[2] + e12 * rtM11; npb[2] = S[2] - e12 * rtM11;
      break;
    case 1:
      npa[0] = S[1] + rtM22; npb[0] = S[1] - rtM22;
      npa[1] = S[4]; npb[1] = S[4];
      npa[2] = S[5] - e02 * rtM00; npb[2] = S[5] + e02 * rtM00;
      break;
    default:
      npa[0] = S[2] + e01 * rtM11; npb[0] = S[2] - e01 * rtM11;
      npa[1] = S[5] + rtM00; npb[1] = S[5] - rtM00;
      npa[2] = S[8]; npb[2] = S[8];
      break;
  }
  const double traceS = S[0] + S[4] + S[8];
  const double v = 2.0 * std::sqrt(1 + traceS - M00 - M11 - M22);
  const double ESii = signd(S[3 * indx + indx]);
  const double r_2 = 2 + traceS + v, nt_2 = 2 + traceS - v;
  const double r = std::sqrt(r_2), n_t = std::sqrt(nt_2);
  const double na_n = norm3(npa), nb_n = norm3(npb);
  double na[3], nb[3];
  for (int i = 0; i < 3; ++i) { na[i] = npa[i] / na_n; nb[i] = npb[i] / nb_n; }
  const double half_nt = 0.5 * n_t, esii_t_r = ESii * r;
  double ta_star[3], tb_star[3];
  for (int i = 0; i < 3; ++i) {
    ta_star[i] = half_nt * (esii_t_r * nb[i] - n_t * na[i]);
    tb_star[i] = half_nt * (esii_t_r * na[i] - n_t * nb[i]);
  }
  motions->resize(4);
  double Ra[9], Rb[9], ta[3], tb[3];
  findRmatFrom_tstar_n(Hn, ta_star, na, v, Ra);
  matvec3(Ra, ta_star, ta);
  findRmatFrom_tstar_n(Hn, tb_star, nb, v, Rb);
  matvec3(Rb, tb_star, tb);
  for (int i = 0; i < 9; ++i) { (*motions)[0].R[i] = Ra[i]; (*motions)[1].R[i] = Ra[i]; (*motions)[2].R[i] = Rb[i]; (*motions)[3].R[i] = Rb[i]; }
  for (int i = 0; i < 3; ++i) {
    (*motions)[0].t[i] = ta[i]; (*motions)[0].n[i] = na[i];
    (*motions)[1].t[i] = -ta[i]; (*motions)[1].n[i] = -na[i];
    (*motions)[2].t[i] = tb[i]; (*motions)[2].n[i] = nb[i];
    (*motions)[3].t[i] = -tb[i]; (*motions)[3].n[i] = -nb[i];
  }
}

double sampsonDistance(const double f_cur[3], const double E[9], const double f_ref[3])
{
  double f_cur_pred[3], f_ref_pred[3];
  matvec3(E, f_ref, f_cur_pred);
  matTvec3(E, f_cur, f_ref_pred);
  const double error = dot3(f_cur, f_cur_pred);
  const double uc[2] = { f_cur_pred[0] / f_cur_pred[2], f_cur_pred[1] / f_cur_pred[2] };
  const double ur[2] = { f_ref_pred[0] / f_ref_pred[2], f_ref_pred[1] / f_ref_pred[2] };
  return error * error / ((uc[0] * uc[0] + uc[1] * uc[1]) + (ur[0] * ur[0] + ur[1] * ur[1]));
}

Homography selectMotion(const double H_cur_ref[9], const double* f_cur, const double* f_ref, const uint8_t* inliers, size_t n, double thresh,
                        double cheirality[4], int* picked)
{
  if (cheirality) for (int i = 0; i < 4; ++i) cheirality[i] = 0.0;
  if (picked) *picked = -1;
  std::vector<CameraMotion> motions;
  decomposeHomography(H_cur_ref, &motions);
  if (motions.size() != 4) return Homography();   // (the reference: CHECK_EQ(rotations.size(), 4u))
  struct Scored { Homography d; int index; };
  std::vector<Scored> decomp(4);
  size_t n_inliers = 0;
  for (size_t i = 0; i < n; ++i) n_inliers += inliers[i] != 0;
  for (int k = 0; k < 4; ++k) {
    Homography& D = decomp[(size_t)k].d;
    decomp[(size_t)k].index = k;
    for (int i = 0; i < 3; ++i) { D.t_cur_ref[i] = motions[(size_t)k].t[i]; D.n_cur[i] = motions[(size_t)k].n[i]; }
    for (int i = 0; i < 9; ++i) D.R_cur_ref[i] = motions[(size_t)k].R[i];
    D.score = 0;   // the plane in front of the camera
    for (size_t i = 0; i < n; ++i) {
      if (!inliers[i]) continue;
      if (dot3(&f_cur[3 * i], D.n_cur) > 0.0) D.score += 1.0;
    }
    if (cheirality) cheirality[k] = D.score;
  }
  std::stable_sort(decomp.begin(), decomp.end(), [](const Scored& lhs, const Scored& rhs) { return lhs.d.score > rhs.d.score; });
  decomp.resize(2);
  if (decomp[1].d.score / decomp[0].d.score < 0.9) {
    decomp.erase(decomp.begin() + 1);   // no ambiguity
  } else {
    const double thresh_squared = thresh * thresh * 4.0;
    for (Scored& s : decomp) {
      Homography& D = s.d;
      D.score = 0.0;
      const double* t = D.t_cur_ref;
      const double sk[9] = { 0, -t[2], t[1], t[2], 0, -t[0], -t[1], t[0], 0 };
      double E[9];
      matmul3(D.R_cur_ref, sk, E);
      for (size_t i = 0; i < n; ++i) {
        const double d = sampsonDistance(&f_cur[3 * i], E, &f_ref[3 * i]);
        D.score += std::min(d, thresh_squared);
      }
    }
    if (decomp[0].d.score < decomp[1].d.score) decomp.erase(decomp.begin() + 1);
    else decomp.erase(decomp.begin());
  }
  decomp[0].d.score = (double)n_inliers;
  if (picked) *picked = decomp[0].index;
  return decomp[0].d;
}

svoh::Quat quaternionFromRotation(const double R[9])
{
  svoh::Quat q;
  const double tr = R[0] + R[4] + R[8];
  if (tr > 0) {
    double t = std::sqrt(tr + 1.0);
    q.w = 0.5 * t; t = 0.5 / t;
    q.x = (R[7] - R[5]) * t; q.y = (R[2] - R[6]) * t; q.z = (R[3] - R[1]) * t;
  } else {
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > R[4 * i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    double t = std::sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0);
    double v[3];
    v[i] = 0.5 * t; t = 0.5 / t;
    q.w = (R[3 * k + j] - R[3 * j + k]) * t;
    v[j] = (R[3 * j + i] + R[3 * i + j]) * t;
    v[k] = (R[3 * k + i] + R[3 * i + k]) * t;
    q.x = v[0]; q.y = v[1]; q.z = v[2];
  }
  return svoh::normalized(q);
}

void triangulateFeatureNonLin(const double R[9], const double t[3], const double feature1[3], const double feature2[3], double xyz[3])
{
  double f2[3];
  matvec3(R, feature2, f2);
  const double b0 = dot3(t, feature1), b1 = dot3(t, f2);
  const double a00 = dot3(feature1, feature1), a10 = dot3(feature1, f2);
  const double a01 = -a10, a11 = -dot3(f2, f2);
  const double det = a00 * a11 - a01 * a10;   // Eigen's 2x2 inverse: adjugate / determinant
  const double l0 = (a11 * b0 - a01 * b1) / det, l1 = (-a10 * b0 + a00 * b1) / det;
  for (int i = 0; i < 3; ++i) xyz[i] = (l0 * feature1[i] + (t[i] + l1 * f2[i])) / 2;
}

double computeInliers(const double* features1, const double* features2, size_t n, const double R_12[9], const double t[3], double reproj_thresh,
                      double error_multiplier2, std::vector<double>* xyz_vec_in_1, std::vector<int>* inliers, std::vector<int>* outliers)
{
  inliers->clear(); outliers->clear();
  xyz_vec_in_1->assign(3 * n, 0.0);
  double tot_error = 0;
  for (size_t j = 0; j < n; ++j) {
    double* X = &(*xyz_vec_in_1)[3 * j];
    triangulateFeatureNonLin(R_12, t, &features1[3 * j], &features2[3 * j], X);
    auto reproj = [&](const double* f1, const double* f2) {
      const double ex = f1[0] / f1[2] - f2[0] / f2[2], ey = f1[1] / f1[2] - f2[1] / f2[2];
      return error_multiplier2 * std::sqrt(ex * ex + ey * ey);
    };
    const double e1 = reproj(&features1[3 * j], X);
    const double d[3] = { X[0] - t[0], X[1] - t[1], X[2] - t[2] };
    double Y[3];
    matTvec3(R_12, d, Y);
    const double e2 = reproj(&features2[3 * j], Y);
    if (e1 > reproj_thresh || e2 > reproj_thresh) outliers->push_back((int)j);
    else { inliers->push_back((int)j); tot_error += e1 + e2; }
  }
  return tot_error;
}

}  // namespace vk

namespace feature_tracking_utils {

double getTracksDisparityPercentile(std::vector<double> disparities, double pivot_ratio)
{
  if (!(pivot_ratio > 0.0 && pivot_ratio < 1.0)) throw std::invalid_argument("pivot_ratio needs to be in (0,1)");
  if (disparities.empty()) return 0.0;
  const size_t pivot = (size_t)std::floor(pivot_ratio * (double)disparities.size());
  std::nth_element(disparities.begin(), disparities.begin() + (long)pivot, disparities.end(), std::greater<double>());
  return disparities[pivot];
}

void getFeatureMatches(const int* track_ids_1, size_t n1, const int* track_ids_2, size_t n2, std::vector<std::pair<size_t, size_t>>* matches_12)
{
  std::unordered_map<int, size_t> trackid_slotid_map;
  for (size_t i = 0; i < n1; ++i)
    if (track_ids_1[i] >= 0) trackid_slotid_map[track_ids_1[i]] = i;
  matches_12->reserve(n2);
  for (size_t i = 0; i < n2; ++i) {
    if (track_ids_2[i] < 0) continue;
    const auto it = trackid_slotid_map.find(track_ids_2[i]);
    if (it != trackid_slotid_map.end()) matches_12->push_back(std::make_pair(it->second, i));
  }
}

}  // namespace feature_tracking_utils

namespace initialization_utils {

namespace {
inline double angleError(const double f1[3], const double f2[3]) { return std::acos(dot3(f1, f2) / (norm3(f1) * norm3(f2))); }
}

void triangulatePoints(const double* f_vec_cur, const double* f_vec_ref, const svoh::Rigid& T_cur_ref, double angle_threshold, bool pinhole,
                       FeatureMatches* matches_cur_ref, std::vector<double>* points_in_cur)
{
  points_in_cur->clear();
  const svoh::Rigid T_ref_cur = svoh::inverse(T_cur_ref);
  double R[9];
  svoh::to_matrix(T_cur_ref.q, R);
  const double t[3] = { T_cur_ref.t.x, T_cur_ref.t.y, T_cur_ref.t.z };
  FeatureMatches kept;
  for (size_t i = 0; i < matches_cur_ref->size(); ++i) {
    const double* f_cur = &f_vec_cur[3 * (*matches_cur_ref)[i].first];
    const double* f_ref = &f_vec_ref[3 * (*matches_cur_ref)[i].second];
    double X[3];
    vk::triangulateFeatureNonLin(R, t, f_cur, f_ref, X);
    const svoh::Vec3 Xr = svoh::transform(T_ref_cur, svoh::Vec3{ X[0], X[1], X[2] });
    const double Xr3[3] = { Xr.x, Xr.y, Xr.z };
    const double e1 = angleError(f_cur, X), e2 = angleError(f_ref, Xr3);
    if (e1 > angle_threshold || e2 > angle_threshold || (pinhole && X[2] < 0.0)) continue;   // an outlier: erased
    kept.push_back((*matches_cur_ref)[i]);
    points_in_cur->insert(points_in_cur->end(), X, X + 3);
  }
  matches_cur_ref->swap(kept);
}

void rescalePoints(const std::vector<double>& points_in_cur, const svoh::Rigid& T_cur_ref, const svoh::Rigid& T_ref_world, double depth_at_current_frame,
                   double* scale, svoh::Rigid* T_cur_world, std::vector<double>* points_in_world)
{
  const size_t n = points_in_cur.size() / 3;
  if (n < 2) throw std::runtime_error("rescaleAndInitializePoints: fewer than two points");   // CHECK_GT(depth_vec.size(), 1u)
  std::vector<double> depth_vec(n);
  for (size_t i = 0; i < n; ++i) depth_vec[i] = norm3(&points_in_cur[3 * i]);
  std::nth_element(depth_vec.begin(), depth_vec.begin() + (long)(n / 2), depth_vec.end());   // vk::getMedian
  const double scene_depth_median = depth_vec[n / 2];
  *scale = depth_at_current_frame / scene_depth_median;
  svoh::Rigid T = svoh::mul(T_cur_ref, T_ref_world);
  const svoh::Vec3 pos_ref = svoh::inverse(T_ref_world).t, pos_cur = svoh::inverse(T).t;
  const svoh::Vec3 p{ pos_ref.x + *scale * (pos_cur.x - pos_ref.x), pos_ref.y + *scale * (pos_cur.y - pos_ref.y), pos_ref.z + *scale * (pos_cur.z - pos_ref.z) };
  const svoh::Vec3 rp = svoh::rotate(T.q, p);
  T.t = svoh::Vec3{ -rp.x, -rp.y, -rp.z };
  *T_cur_world = T;
  const svoh::Rigid T_world_cur = svoh::inverse(T);
  points_in_world->resize(3 * n);
  for (size_t i = 0; i < n; ++i) {
    const svoh::Vec3 w = svoh::transform(T_world_cur, svoh::Vec3{ points_in_cur[3 * i] * *scale, points_in_cur[3 * i + 1] * *scale, points_in_cur[3 * i + 2] * *scale });
    (*points_in_world)[3 * i] = w.x; (*points_in_world)[3 * i + 1] = w.y; (*points_in_world)[3 * i + 2] = w.z;
  }
}

}  // namespace initialization_utils

#ifndef SVOH_INIT_MATH_ONLY

namespace vk {

Homography estimateHomography(svoh_ctx* ctx, const std::vector<double>& f_cur, const std::vector<double>& f_ref, double focal_length,
                              double reproj_error_thresh, size_t min_num_inliers, uint64_t seed, int n_hypotheses, svoh_homography_result* result,
                              double* ms_kernel)
{
  if (f_cur.size() != f_ref.size() || f_cur.size() % 3 != 0) throw std::runtime_error("estimateHomography: f_cur and f_ref differ in size");
  const size_t N = f_cur.size() / 3;
  if (N > 1024) throw std::runtime_error("estimateHomography: more than 1024 matches (svoh_homography_ransac_batch's limit)");
  const double thresh = reproj_error_thresh / focal_length;
  std::vector<double> uv_ref(2 * N), uv_cur(2 * N);
  for (size_t i = 0; i < N; ++i) {   // vk::project2
    uv_ref[2 * i] = f_ref[3 * i] / f_ref[3 * i + 2]; uv_ref[2 * i + 1] = f_ref[3 * i + 1] / f_ref[3 * i + 2];
    uv_cur[2 * i] = f_cur[3 * i] / f_cur[3 * i + 2]; uv_cur[2 * i + 1] = f_cur[3 * i + 1] / f_cur[3 * i + 2];
  }
  svoh_init_options opt{};
  opt.n_hypotheses = n_hypotheses;
  svoh_homography_problem pb{};
  pb.n = (int32_t)N; pb.uv_ref = uv_ref.data(); pb.uv_cur = uv_cur.data(); pb.thresh = thresh; pb.seed = seed;
  svoh_homography_result res{};
  std::vector<uint8_t> inliers(N ? N : 1, 0);
  if (svoh_homography_ransac_batch(ctx, &opt, 1, &pb, &res, inliers.data()) != SVOH_OK)
    throw std::runtime_error(std::string("svoh_homography_ransac_batch: ") + svoh_last_error_string(ctx));
  if (result) *result = res;
  if (ms_kernel) {
    float ms = -1.0f;
    *ms_kernel = svoh_last_kernel_ms(ctx, &ms) == SVOH_OK ? (double)ms : -1.0;
  }
  if (res.status != SVOH_HOMOGRAPHY_OK || (size_t)res.n_inliers < min_num_inliers) return Homography();   // score zero
  return selectMotion(res.H, f_cur.data(), f_ref.data(), inliers.data(), N, thresh);
}

}  // namespace vk

size_t estimateTranslation(svoh_ctx* ctx, const std::vector<double>& f_cur, const std::vector<double>& f_ref, const double R_cur_ref[9], double thresh,
                           uint64_t seed, int n_hypotheses, double t_cur_ref[3], std::vector<uint8_t>* inliers, svoh_translation_result* result,
                           double* ms_kernel)
{
  if (f_cur.size() != f_ref.size() || f_cur.size() % 3 != 0) throw std::runtime_error("estimateTranslation: f_cur and f_ref differ in size");
  const size_t N = f_cur.size() / 3;
  if (N > 1024) throw std::runtime_error("estimateTranslation: more than 1024 matches (svoh_translation_ransac_batch's limit)");
  svoh_init_options opt{};
  opt.n_hypotheses = n_hypotheses;
  svoh_translation_problem pb{};
  pb.n = (int32_t)N; pb.f_cur = f_cur.data(); pb.f_ref = f_ref.data(); pb.thresh = thresh; pb.seed = seed;
  for (int i = 0; i < 9; ++i) pb.R_cur_ref[i] = R_cur_ref[i];
  svoh_translation_result res{};
  std::vector<uint8_t> mask(N ? N : 1, 0);
  if (svoh_translation_ransac_batch(ctx, &opt, 1, &pb, &res, mask.data()) != SVOH_OK)
    throw std::runtime_error(std::string("svoh_translation_ransac_batch: ") + svoh_last_error_string(ctx));
  if (result) *result = res;
  if (ms_kernel) {
    float ms = -1.0f;
    *ms_kernel = svoh_last_kernel_ms(ctx, &ms) == SVOH_OK ? (double)ms : -1.0;
  }
  for (int i = 0; i < 3; ++i) t_cur_ref[i] = res.t[i];   // zero without a model
  if (inliers) { mask.resize(N); inliers->swap(mask); }
  return res.status == SVOH_TRANSLATION_OK ? (size_t)res.n_inliers : 0;
}

size_t estimateRelativePose(svoh_ctx* ctx, const std::vector<double>& f_cur, const std::vector<double>& f_ref, double thresh, uint64_t seed,
                            int n_hypotheses, double R_cur_ref[9], double t_cur_ref[3], std::vector<uint8_t>* inliers, svoh_essential_result* result,
                            double* ms_kernel)
{
  if (f_cur.size() != f_ref.size() || f_cur.size() % 3 != 0) throw std::runtime_error("estimateRelativePose: f_cur and f_ref differ in size");
  const size_t N = f_cur.size() / 3;
  if (N > 1024) throw std::runtime_error("estimateRelativePose: more than 1024 matches (svoh_essential_ransac_batch's limit)");
  svoh_init_options opt{};
  opt.n_hypotheses = n_hypotheses;
  svoh_essential_problem pb{};
  pb.n = (int32_t)N; pb.f_cur = f_cur.data(); pb.f_ref = f_ref.data(); pb.thresh = thresh; pb.seed = seed;
  svoh_essential_result res{};
  std::vector<uint8_t> mask(N ? N : 1, 0);
  if (svoh_essential_ransac_batch(ctx, &opt, 1, &pb, &res, mask.data()) != SVOH_OK)
    throw std::runtime_error(std::string("svoh_essential_ransac_batch: ") + svoh_last_error_string(ctx));
  if (result) *result = res;
  if (ms_kernel) {
    float ms = -1.0f;
    *ms_kernel = svoh_last_kernel_ms(ctx, &ms) == SVOH_OK ? (double)ms : -1.0;
  }
  for (int i = 0; i < 9; ++i) R_cur_ref[i] = res.R[i];   // zero without a model
  for (int i = 0; i < 3; ++i) t_cur_ref[i] = res.t[i];
  if (inliers) { mask.resize(N); inliers->swap(mask); }
  return res.status == SVOH_ESSENTIAL_OK ? (size_t)res.n_inliers : 0;
}

namespace initialization_utils {

void triangulatePoints(const Frame& frame_cur, const Frame& frame_ref, const Transformation& T_cur_ref, double reprojection_threshold,
                       FeatureMatches& matches_cur_ref, std::vector<double>& points_in_cur)
{
  // Frame::getAngleError (pinhole_projection.hpp:72-76)
  const double angle_threshold = std::atan(reprojection_threshold / (2.0 * frame_cur.cam.fx)) + std::atan(reprojection_threshold / (2.0 * frame_cur.cam.fy));
  // (every model of svoh_camera is a pinhole projection with a distortion: Camera::Type::kPinhole)
  triangulatePoints(frame_cur.f_vec_.data(), frame_ref.f_vec_.data(), T_cur_ref, angle_threshold, true, &matches_cur_ref, &points_in_cur);
}

namespace {
// Frame::resizeFeatureStorage for the columns a tracked frame does not carry yet
void completeFeatureStorage(Frame& f)
{
  const size_t n = f.num_features_;
  f.grad_vec_.resize(2 * n, 0.0);
  f.level_vec_.resize(n, 0);
  f.type_vec_.resize(n, SVOH_FT_CORNER);
  f.score_vec_.resize(n, -1.0);
  f.track_id_vec_.resize(n, -1);
  f.invmu_sigma2_a_b_vec_.resize(4 * n, 0.0);
  f.landmark_vec_.resize(n);
  f.seed_ref_vec_.resize(n);
}
}  // namespace

double rescaleAndInitializePoints(const FramePtr& frame_cur, const FramePtr& frame_ref, const FeatureMatches& matches_cur_ref,
                                  const std::vector<double>& points_in_cur, const Transformation& T_cur_ref, double depth_at_current_frame)
{
  double scale = 0.0;
  Transformation T_cur_world;
  std::vector<double> world;
  rescalePoints(points_in_cur, T_cur_ref, frame_ref->T_f_w_, depth_at_current_frame, &scale, &T_cur_world, &world);
  frame_cur->T_f_w_ = T_cur_world;
  completeFeatureStorage(*frame_cur);
  completeFeatureStorage(*frame_ref);
  for (size_t i = 0; i < matches_cur_ref.size(); ++i) {
    const size_t ic = matches_cur_ref[i].first, ir = matches_cur_ref[i].second;
    const int point_id_cur = frame_cur->track_id_vec_.at(ic), point_id_ref = frame_ref->track_id_vec_.at(ir);
    if (point_id_cur != point_id_ref) throw std::runtime_error("rescaleAndInitializePoints: a match joins two tracks");   // CHECK_EQ
    PointPtr new_point(new Point);
    new_point->id_ = point_id_cur;
    new_point->pos_ = svoh::Vec3{ world[3 * i], world[3 * i + 1], world[3 * i + 2] };
    frame_cur->landmark_vec_.at(ic) = new_point;
    frame_ref->landmark_vec_.at(ir) = new_point;
    new_point->addObservation(frame_ref, ir);
    new_point->addObservation(frame_cur, ic);
  }
  return scale;
}

bool triangulateAndInitializePoints(const FramePtr& frame_cur, const FramePtr& frame_ref, const Transformation& T_cur_ref, double reprojection_threshold,
                                    double depth_at_current_frame, size_t min_inliers_threshold, FeatureMatches& matches_cur_ref, double* scale)
{
  std::vector<double> points_in_cur;
  triangulatePoints(*frame_cur, *frame_ref, T_cur_ref, reprojection_threshold, matches_cur_ref, points_in_cur);
  if (matches_cur_ref.size() < min_inliers_threshold || matches_cur_ref.size() < 2) return false;
  const double s = rescaleAndInitializePoints(frame_cur, frame_ref, matches_cur_ref, points_in_cur, T_cur_ref, depth_at_current_frame);
  if (scale) *scale = s;
  return true;
}

}  // namespace initialization_utils

namespace frame_utils {

bool getSceneDepth(const Frame& frame, double& depth_median, double& depth_min, double& depth_max)
{
  std::vector<double> depth_vec;
  depth_min = std::numeric_limits<double>::max();
  depth_max = 0;
  const svoh::Vec3 ref_pos = frame.pos();
  for (size_t i = 0; i < frame.num_features_; ++i) {
    double depth = 0;
    if (i < frame.landmark_vec_.size() && frame.landmark_vec_[i]) {
      const svoh::Vec3 p = svoh::transform(frame.T_f_w_, frame.landmark_vec_[i]->pos_);
      depth = std::sqrt(p.x * p.x + p.y * p.y + p.z * p.z);
    } else if (i < frame.seed_ref_vec_.size() && frame.seed_ref_vec_[i].keyframe) {
      const Frame::SeedRef& sr = frame.seed_ref_vec_[i];
      const Frame& kf = *sr.keyframe;
      const double d = kf.getSeedDepth((size_t)sr.seed_id);   // getSeedPosInFrame: f * depth
      const svoh::Vec3 pos = svoh::transform(svoh::inverse(kf.T_f_w_), svoh::Vec3{ kf.f_vec_[3 * sr.seed_id] * d, kf.f_vec_[3 * sr.seed_id + 1] * d, kf.f_vec_[3 * sr.seed_id + 2] * d });
      const double dx = pos.x - ref_pos.x, dy = pos.y - ref_pos.y, dz = pos.z - ref_pos.z;
      depth = std::sqrt(dx * dx + dy * dy + dz * dz);
    } else {
      continue;
    }
    depth_vec.push_back(depth);
    depth_min = std::min(depth, depth_min);
    depth_max = std::max(depth, depth_max);
  }
  if (depth_vec.empty()) return false;
  std::nth_element(depth_vec.begin(), depth_vec.begin() + (long)(depth_vec.size() / 2), depth_vec.end());
  depth_median = depth_vec[depth_vec.size() / 2];
  return true;
}

}  // namespace frame_utils

// ---- the tracker's two queries the initialiser makes (feature_tracker.cpp:202-226) ----
void FeatureTrackerHip::getNumTrackedAndDisparityPerFrame(double pivot_ratio, std::vector<size_t>* num_tracked, std::vector<double>* disparity) const
{
  if (!num_tracked || !disparity) throw std::runtime_error("FeatureTrackerHip::getNumTrackedAndDisparityPerFrame: NULL argument");
  num_tracked->resize(bundle_size_);
  disparity->resize(bundle_size_);
  for (size_t i = 0; i < bundle_size_; ++i) {
    (*num_tracked)[i] = active_tracks_[i].size();
    std::vector<double> d;
    d.reserve(active_tracks_[i].size());
    for (const FeatureTrack& track : active_tracks_[i]) {   // FeatureTrack::getDisparity: |first px - last px|
      const double* a = track.front().getPx();
      const double* b = track.back().getPx();
      d.push_back(std::sqrt((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1])));
    }
    (*disparity)[i] = feature_tracking_utils::getTracksDisparityPercentile(std::move(d), pivot_ratio);
  }
}

FrameBundle::Ptr FeatureTrackerHip::getOldestFrameInTrack(size_t frame_index) const
{
  if (frame_index >= active_tracks_.size() || active_tracks_[frame_index].empty() || active_tracks_[frame_index].front().empty())
    throw std::runtime_error("FeatureTrackerHip::getOldestFrameInTrack: no active track");
  return active_tracks_[frame_index].front().at(0).getFrameBundle();
}

// ---- AbstractInitialization -------------------------------------------------------------------------------------------
AbstractInitializationHip::AbstractInitializationHip(svoh_ctx* ctx, const InitializationOptions& init_options, const FeatureTrackerOptions& tracker_options,
                                                     const std::shared_ptr<DetectorHip>& detector, const char* who)
    : ctx_(ctx), options_(init_options), tracker_(ctx, tracker_options, 1)
{
  if (!ctx_) throw std::runtime_error(std::string(who) + ": NULL svoh_ctx (no CPU fallback exists)");
  tracker_.setDetectors({ detector });
}

void AbstractInitializationHip::reset()
{
  frames_ref_.reset();
  have_rotation_prior_ = false;
  have_depth_prior_ = false;
  tracker_.reset();
}

namespace {
void clearFeatureStorage(Frame& frame)
{
  frame.num_features_ = 0;
  frame.px_vec_.clear(); frame.f_vec_.clear(); frame.grad_vec_.clear(); frame.level_vec_.clear();
  frame.type_vec_.clear(); frame.score_vec_.clear(); frame.track_id_vec_.clear();
  frame.landmark_vec_.clear(); frame.seed_ref_vec_.clear(); frame.invmu_sigma2_a_b_vec_.clear();
}
}  // namespace

bool AbstractInitializationHip::trackFeaturesAndCheckDisparity(const FrameBundle::Ptr& frames)
{
  tracker_.trackFrameBundle(frames);
  std::vector<size_t> num_tracked;
  std::vector<double> disparity;
  tracker_.getNumTrackedAndDisparityPerFrame(options_.init_disparity_pivot_ratio, &num_tracked, &disparity);
  size_t num_tracked_tot = 0;
  double avg_disparity = 0.0;
  for (size_t v : num_tracked) num_tracked_tot += v;
  for (double v : disparity) avg_disparity += v;
  avg_disparity /= (double)disparity.size();
  stats_.n_tracked = num_tracked_tot;
  stats_.disparity = avg_disparity;
  if (num_tracked_tot < options_.init_min_features) {
    tracker_.resetActiveTracks();
    for (const FramePtr& frame : frames->frames_) clearFeatureStorage(*frame);
    tracker_.initializeNewTracks(frames);
    frames_ref_ = frames;
    R_ref_world_ = R_cur_world_;
    return false;
  }
  if (avg_disparity < options_.init_min_disparity) return false;
  return true;
}

// ---- HomographyInit ---------------------------------------------------------------------------------------------------
HomographyInitHip::HomographyInitHip(svoh_ctx* ctx, const InitializationOptions& init_options, const FeatureTrackerOptions& tracker_options,
                                     const std::shared_ptr<DetectorHip>& detector)
    : AbstractInitializationHip(ctx, init_options, tracker_options, detector, "HomographyInitHip")
{
}

InitResult HomographyInitHip::addFrameBundle(const FrameBundle::Ptr& frames_cur)
{
  stats_ = Statistics();
  if (!frames_cur || frames_cur->size() != 1) throw std::runtime_error("HomographyInitHip: one camera per bundle");
  if (!trackFeaturesAndCheckDisparity(frames_cur)) return InitResult::kTracking;

  const FrameBundle::Ptr frames_ref = tracker_.getOldestFrameInTrack(0);
  const Frame& frame_ref = *frames_ref->at(0);
  const Frame& frame_cur = *frames_cur->at(0);
  initialization_utils::FeatureMatches matches_cur_ref;
  feature_tracking_utils::getFeatureMatches(frame_cur.track_id_vec_.data(), frame_cur.num_features_, frame_ref.track_id_vec_.data(), frame_ref.num_features_, &matches_cur_ref);
  const size_t n = matches_cur_ref.size();
  std::vector<double> f_cur(3 * n), f_ref(3 * n);
  for (size_t i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) {
      f_cur[3 * i + k] = frame_cur.f_vec_[3 * matches_cur_ref[i].first + k];
      f_ref[3 * i + k] = frame_ref.f_vec_[3 * matches_cur_ref[i].second + k];
    }

  // the model (getErrorMultiplier of a pinhole projection: |fx|)
  double ms = -1.0;
  const vk::Homography H_cur_ref = vk::estimateHomography(ctx_, f_cur, f_ref, std::fabs(frames_ref_->at(0)->cam.fx), options_.reproj_error_thresh,
                                                          options_.init_min_inliers, options_.seed, options_.n_hypotheses, nullptr, &ms);
  stats_.ms_ransac = ms;
  stats_.n_inliers = (size_t)H_cur_ref.score;
  if (H_cur_ref.score < (double)options_.init_min_inliers) {
    reset();   // (deviation 3: the caller goes on with the next frame)
    return InitResult::kFailure;
  }
  T_cur_from_ref_ = Transformation{ vk::quaternionFromRotation(H_cur_ref.R_cur_ref), svoh::Vec3{ H_cur_ref.t_cur_ref[0], H_cur_ref.t_cur_ref[1], H_cur_ref.t_cur_ref[2] } };

  double scale = 0.0;
  if (initialization_utils::triangulateAndInitializePoints(frames_cur->at(0), frames_ref_->at(0), T_cur_from_ref_, options_.reproj_error_thresh,
                                                           depth_at_current_frame_, options_.init_min_inliers, matches_cur_ref, &scale)) {
    stats_.n_triangulated = matches_cur_ref.size();
    stats_.scale = scale;
    return InitResult::kSuccess;
  }
  stats_.n_triangulated = matches_cur_ref.size();
  // restart
  tracker_.reset();
  clearFeatureStorage(*frames_cur->at(0));
  return InitResult::kTracking;
}

// ---- TwoPointInit -----------------------------------------------------------------------------------------------------
TwoPointInitHip::TwoPointInitHip(svoh_ctx* ctx, const InitializationOptions& init_options, const FeatureTrackerOptions& tracker_options,
                                 const std::shared_ptr<DetectorHip>& detector)
    : AbstractInitializationHip(ctx, init_options, tracker_options, detector, "TwoPointInitHip")
{
}

InitResult TwoPointInitHip::addFrameBundle(const FrameBundle::Ptr& frames_cur)
{
  stats_ = Statistics();
  if (!have_rotation_prior_) return InitResult::kFailure;   // ("TwoPointInit has no rotation prior.")
  have_rotation_prior_ = false;
  if (!frames_cur || frames_cur->size() != 1) throw std::runtime_error("TwoPointInitHip: one camera per bundle");
  if (!trackFeaturesAndCheckDisparity(frames_cur)) return InitResult::kTracking;

  const FrameBundle::Ptr frames_ref = tracker_.getOldestFrameInTrack(0);
  const Frame& frame_ref = *frames_ref->at(0);
  const Frame& frame_cur = *frames_cur->at(0);
  initialization_utils::FeatureMatches matches_cur_ref;
  feature_tracking_utils::getFeatureMatches(frame_cur.track_id_vec_.data(), frame_cur.num_features_, frame_ref.track_id_vec_.data(), frame_ref.num_features_, &matches_cur_ref);
  const size_t n = matches_cur_ref.size();
  std::vector<double> f_cur(3 * n), f_ref(3 * n);   // initialization_utils::copyBearingVectors
  for (size_t i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) {
      f_cur[3 * i + k] = frame_cur.f_vec_[3 * matches_cur_ref[i].first + k];
      f_ref[3 * i + k] = frame_ref.f_vec_[3 * matches_cur_ref[i].second + k];
    }

  // the model: 1 - cos(Frame::getAngleError(reproj_error_thresh)) (pinhole_projection.hpp:72-76), R_cur_ref from the two priors
  const double angle_error = std::atan(options_.reproj_error_thresh / (2.0 * frame_cur.cam.fx)) + std::atan(options_.reproj_error_thresh / (2.0 * frame_cur.cam.fy));
  const double inlier_threshold = 1.0 - std::cos(angle_error);
  const svoh::Quat q_cur_ref = svoh::normalized(svoh::mul(R_cur_world_, svoh::Quat{ R_ref_world_.w, -R_ref_world_.x, -R_ref_world_.y, -R_ref_world_.z }));
  double R_cur_ref[9], t[3];
  svoh::to_matrix(q_cur_ref, R_cur_ref);
  double ms = -1.0;
  const size_t n_inliers = estimateTranslation(ctx_, f_cur, f_ref, R_cur_ref, inlier_threshold, options_.seed, options_.n_hypotheses, t, nullptr, nullptr, &ms);
  stats_.ms_ransac = ms;
  stats_.n_inliers = n_inliers;
  if (n_inliers < options_.init_min_inliers) return InitResult::kNoKeyframe;
  T_cur_from_ref_ = Transformation{ q_cur_ref, svoh::Vec3{ t[0], t[1], t[2] } };

  double scale = 0.0;
  const bool ok = initialization_utils::triangulateAndInitializePoints(frames_cur->at(0), frames_ref->at(0), T_cur_from_ref_, options_.reproj_error_thresh,
                                                                       depth_at_current_frame_, options_.init_min_inliers, matches_cur_ref, &scale);
  stats_.n_triangulated = matches_cur_ref.size();
  if (!ok) return InitResult::kFailure;
  stats_.scale = scale;
  return InitResult::kSuccess;
}

// ---- FivePointInit ----------------------------------------------------------------------------------------------------
FivePointInitHip::FivePointInitHip(svoh_ctx* ctx, const InitializationOptions& init_options, const FeatureTrackerOptions& tracker_options,
                                   const std::shared_ptr<DetectorHip>& detector)
    : AbstractInitializationHip(ctx, init_options, tracker_options, detector, "FivePointInitHip")
{
}

InitResult FivePointInitHip::addFrameBundle(const FrameBundle::Ptr& frames_cur)
{
  stats_ = Statistics();
  if (!frames_cur || frames_cur->size() != 1) throw std::runtime_error("FivePointInitHip: one camera per bundle");
  if (!trackFeaturesAndCheckDisparity(frames_cur)) return InitResult::kTracking;

  const FrameBundle::Ptr frames_ref = tracker_.getOldestFrameInTrack(0);
  const Frame& frame_ref = *frames_ref->at(0);
  const Frame& frame_cur = *frames_cur->at(0);
  initialization_utils::FeatureMatches matches_cur_ref;
  feature_tracking_utils::getFeatureMatches(frame_cur.track_id_vec_.data(), frame_cur.num_features_, frame_ref.track_id_vec_.data(), frame_ref.num_features_, &matches_cur_ref);
  const size_t n = matches_cur_ref.size();
  std::vector<double> f_cur(3 * n), f_ref(3 * n);   // initialization_utils::copyBearingVectors
  for (size_t i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) {
      f_cur[3 * i + k] = frame_cur.f_vec_[3 * matches_cur_ref[i].first + k];
      f_ref[3 * i + k] = frame_ref.f_vec_[3 * matches_cur_ref[i].second + k];
    }

  // the model: 1 - cos(Frame::getAngleError(reproj_error_thresh)) (pinhole_projection.hpp:72-76)
  const double angle_error = std::atan(options_.reproj_error_thresh / (2.0 * frame_cur.cam.fx)) + std::atan(options_.reproj_error_thresh / (2.0 * frame_cur.cam.fy));
  const double inlier_threshold = 1.0 - std::cos(angle_error);
  double R_cur_ref[9], t[3], ms = -1.0;
  const size_t n_inliers = estimateRelativePose(ctx_, f_cur, f_ref, inlier_threshold, options_.seed, options_.n_hypotheses, R_cur_ref, t, nullptr, nullptr, &ms);
  stats_.ms_ransac = ms;
  stats_.n_inliers = n_inliers;
  if (n_inliers < options_.init_min_inliers) return InitResult::kNoKeyframe;   // (no model: zero inliers)
  T_cur_from_ref_ = Transformation{ svoh::normalized(vk::quaternionFromRotation(R_cur_ref)), svoh::Vec3{ t[0], t[1], t[2] } };

  double scale = 0.0;
  const bool ok = initialization_utils::triangulateAndInitializePoints(frames_cur->at(0), frames_ref->at(0), T_cur_from_ref_, options_.reproj_error_thresh,
                                                                       depth_at_current_frame_, options_.init_min_inliers, matches_cur_ref, &scale);
  stats_.n_triangulated = matches_cur_ref.size();
  if (!ok) return InitResult::kFailure;
  stats_.scale = scale;
  return InitResult::kSuccess;
}

#endif  // SVOH_INIT_MATH_ONLY

}  // namespace svo_hip
