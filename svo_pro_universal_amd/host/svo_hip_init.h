// svo_hip_init.h -- the mono bootstrap: what FrameHandlerMono::processFirstFrame runs before there is a map
// ("Homography initialiser").  Counterparts in the reference:
//   svo::HomographyInit::addFrameBundle            src/svo/src/initialization.cpp:86-161
//   svo::TwoPointInit::addFrameBundle              src/svo/src/initialization.cpp:164-289
//   svo::FivePointInit::addFrameBundle             src/svo/src/initialization.cpp:292-359
//   vk::estimateHomography                          src/vikit/vikit_common/src/homography.cpp:19-136
//   HomographyDecomp::removeScale, HomographyDecompInria::decompose
//                                                   src/vikit/vikit_common/include/vikit/homography_decomp.h:121-126, 283-430
//   vk::triangulateFeatureNonLin, vk::computeInliers, vk::sampsonDistance
//                                                   src/vikit/vikit_common/src/math_utils.cpp:14-33, 66-98, 193-205
//   initialization_utils::triangulatePoints, rescaleAndInitializePoints      initialization.cpp:756-840
//   feature_tracking_utils::getTracksDisparityPercentile, getFeatureMatches  src/svo_tracker/src/feature_tracking_utils.cpp:10-61
// Same names and argument meaning.  The one part that is NOT the reference's is the estimator inside estimateHomography:
// cv::findHomography's RANSAC cannot be restated, svoh_homography_ransac_batch (include/svo_hip.h) stands in its place.
//
// The maths of this file makes no device call and needs nothing but this header and svoh_math.h: a CPU program compiles
// svo_hip_init.cpp with -DSVOH_INIT_MATH_ONLY and links nothing else (tests/cpp_init).  What runs on the device
// (estimateHomography, estimateTranslation, estimateRelativePose, HomographyInitHip, TwoPointInitHip, FivePointInitHip) is left out of such a build.
#pragma once

#include <cstddef>
#include <cstdint>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../csrc/svoh_math.h"
#ifndef SVOH_INIT_MATH_ONLY
#include "svo_hip_host.h"
#endif

namespace svo_hip {

namespace vk {

// vk::Homography (vikit/homography.h): score 0 = no model
struct Homography {
  double t_cur_ref[3] = { 0, 0, 0 };
  double R_cur_ref[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 };   // row-major
  double n_cur[3] = { 0, 0, 0 };
  double score = 0.0;
};
// HomographyDecomp's CameraMotion
struct CameraMotion { double R[9]; double t[3]; double n[3]; };

// the singular values of a 3x3 matrix in descending order (square roots of the eigenvalues of H^T H, cyclic Jacobi)
void singularValues3(const double H[9], double sv[3]);
// cv::decomposeHomographyMat with K = I as the reference carries it: removeScale (division by the middle singular value),
// then HomographyDecompInria::decompose.  Four motions, or ONE (R = H, t = n = 0) when H is a rotation up to 1e-3.
void decomposeHomography(const double H[9], std::vector<CameraMotion>* motions);
double sampsonDistance(const double f_cur[3], const double E_cur_ref[9], const double f_ref[3]);
// homography.cpp:64-135: decomposition, cheirality scores over the inliers, stable sort, the 0.9 ratio, the capped Sampson
// sums.  f_cur / f_ref: 3 x n bearing vectors, inliers: n flags, thresh = reproj_error_thresh / focal_length.
// A decomposition that does not yield four motions (a pure rotation) gives score 0 -- the reference's CHECK_EQ aborts there.
// cheirality (may be NULL): the four scores in the decomposition's order; picked (may be NULL): the chosen motion's index.
Homography selectMotion(const double H_cur_ref[9], const double* f_cur, const double* f_ref, const uint8_t* inliers, size_t n,
                        double thresh, double cheirality[4] = nullptr, int* picked = nullptr);
// Transformation(Quaternion(R), t): a rotation matrix (row-major) as a unit quaternion, by the branches of Eigen's conversion
svoh::Quat quaternionFromRotation(const double R[9]);
void triangulateFeatureNonLin(const double R[9], const double t[3], const double feature1[3], const double feature2[3], double xyz[3]);
// vk::computeInliers: the indices whose two reprojection errors are both <= reproj_thresh; returns the summed error
double computeInliers(const double* features1, const double* features2, size_t n, const double R_12[9], const double t[3],
                      double reproj_thresh, double error_multiplier2, std::vector<double>* xyz_vec_in_1, std::vector<int>* inliers,
                      std::vector<int>* outliers);

}  // namespace vk

namespace feature_tracking_utils {
// the percentile of the tracks' disparities (|first px - last px|): the element at floor(pivot_ratio * n) in descending order
double getTracksDisparityPercentile(std::vector<double> disparities, double pivot_ratio);
// pairs (slot in frame 1, slot in frame 2) of the track ids (>= 0) both frames carry, in frame 2's order
void getFeatureMatches(const int* track_ids_1, size_t n1, const int* track_ids_2, size_t n2, std::vector<std::pair<size_t, size_t>>* matches_12);
}  // namespace feature_tracking_utils

namespace initialization_utils {
using FeatureMatches = std::vector<std::pair<size_t, size_t>>;   // (slot in cur, slot in ref)
// triangulatePoints on bare columns: matches that fail the angle test (or lie behind a pinhole camera) are erased,
// points_in_cur receives 3 doubles per remaining match
void triangulatePoints(const double* f_vec_cur, const double* f_vec_ref, const svoh::Rigid& T_cur_ref, double angle_threshold, bool pinhole,
                       FeatureMatches* matches_cur_ref, std::vector<double>* points_in_cur);
// rescaleAndInitializePoints without the bookkeeping: the scale (depth_at_current_frame / median |point|), the current
// frame's pose with that scale, the points in the world
void rescalePoints(const std::vector<double>& points_in_cur, const svoh::Rigid& T_cur_ref, const svoh::Rigid& T_ref_world, double depth_at_current_frame,
                   double* scale, svoh::Rigid* T_cur_world, std::vector<double>* points_in_world);
}  // namespace initialization_utils

#ifndef SVOH_INIT_MATH_ONLY

namespace vk {
// vk::estimateHomography with svoh_homography_ransac_batch where the reference calls cv::findHomography: project2 of the
// bearing vectors on the host, the kernel (n_hypotheses hypotheses from `seed`), the kernel's inlier mask and count for
// homography.cpp:47-56, then selectMotion.  More than 1024 matches: std::runtime_error.  ms_kernel (may be NULL): the
// kernel's device time when kernel timing is on, else -1.
Homography estimateHomography(svoh_ctx* ctx, const std::vector<double>& f_cur, const std::vector<double>& f_ref, double focal_length,
                              double reproj_error_thresh, size_t min_num_inliers, uint64_t seed, int n_hypotheses = 2000,
                              svoh_homography_result* result = nullptr, double* ms_kernel = nullptr);
}  // namespace vk

// The model of TwoPointInit (initialization.cpp:244-266) with svoh_translation_ransac_batch where the reference runs
// opengv's RANSAC: the unit translation t_cur_ref under the known R_cur_ref (row-major) from unit bearing vectors
// (3 doubles a match), thresh = 1 - cos(angle error), n_hypotheses hypotheses from `seed`.  Returns the number of
// inliers (0: no model; t is then zero); inliers (may be NULL): one flag per match.  More than 1024 matches:
// std::runtime_error.  ms_kernel (may be NULL): the kernel's device time when kernel timing is on, else -1.
size_t estimateTranslation(svoh_ctx* ctx, const std::vector<double>& f_cur, const std::vector<double>& f_ref, const double R_cur_ref[9],
                           double thresh, uint64_t seed, int n_hypotheses, double t_cur_ref[3], std::vector<uint8_t>* inliers = nullptr,
                           svoh_translation_result* result = nullptr, double* ms_kernel = nullptr);

// The model of FivePointInit (initialization.cpp:313-337) with svoh_essential_ransac_batch where the reference runs
// opengv's RANSAC over Nister's solver: R_cur_ref (row-major) and the unit translation t_cur_ref from unit bearing vectors
// (3 doubles a match), thresh = 1 - cos(angle error), n_hypotheses hypotheses from `seed`.  Returns the number of inliers
// (0: no model; R and t are then zero); inliers (may be NULL): one flag per match.  More than 1024 matches:
// std::runtime_error.  ms_kernel (may be NULL): the kernel's device time when kernel timing is on, else -1.
size_t estimateRelativePose(svoh_ctx* ctx, const std::vector<double>& f_cur, const std::vector<double>& f_ref, double thresh, uint64_t seed,
                            int n_hypotheses, double R_cur_ref[9], double t_cur_ref[3], std::vector<uint8_t>* inliers = nullptr,
                            svoh_essential_result* result = nullptr, double* ms_kernel = nullptr);

namespace initialization_utils {
// the Frame forms (initialization.cpp:729-840): landmarks are made and hung on both frames, the current frame gets its pose
void triangulatePoints(const Frame& frame_cur, const Frame& frame_ref, const Transformation& T_cur_ref, double reprojection_threshold,
                       FeatureMatches& matches_cur_ref, std::vector<double>& points_in_cur);
double rescaleAndInitializePoints(const FramePtr& frame_cur, const FramePtr& frame_ref, const FeatureMatches& matches_cur_ref,
                                  const std::vector<double>& points_in_cur, const Transformation& T_cur_ref, double depth_at_current_frame);
bool triangulateAndInitializePoints(const FramePtr& frame_cur, const FramePtr& frame_ref, const Transformation& T_cur_ref, double reprojection_threshold,
                                    double depth_at_current_frame, size_t min_inliers_threshold, FeatureMatches& matches_cur_ref, double* scale = nullptr);
}  // namespace initialization_utils

namespace frame_utils {
// frame.cpp:388-425: depths of the frame's landmarks and seed references
bool getSceneDepth(const Frame& frame, double& depth_median, double& depth_min, double& depth_max);
}

enum class InitResult { kFailure, kNoKeyframe, kTracking, kSuccess };   // initialization.h
enum class InitializerType { kHomography, kTwoPoint, kFivePoint, kOneShot, kArrayGeometric, kArrayOptimization };

// InitializationOptions with the defaults of svo_factory.cpp:178-195
struct InitializationOptions {
  InitializerType init_type = InitializerType::kFivePoint;
  std::string init_method = "FivePoint";   // the key as the file has it (an unknown method is kept, and refused by whoever needs one)
  size_t init_min_features = 100;
  double init_min_features_factor = 2.0;
  size_t init_min_tracked = 80;
  size_t init_min_inliers = 70;
  double init_min_disparity = 40.0;
  double init_disparity_pivot_ratio = 0.5;
  double reproj_error_thresh = 2.0;
  int n_hypotheses = 2000;                 // the estimator's K (not a key of the reference)
  uint64_t seed = 12345;                   // ... and its seed: the same frames give the same map
};

// What the reference's initialisers share (AbstractInitialization, initialization.h; initialization.cpp:76-113): the tracker,
// the reference bundle, the priors, and the step every one of them starts with.
class AbstractInitializationHip {
 public:
  AbstractInitializationHip(svoh_ctx* ctx, const InitializationOptions& init_options, const FeatureTrackerOptions& tracker_options,
                            const std::shared_ptr<DetectorHip>& detector, const char* who);
  virtual ~AbstractInitializationHip() = default;
  virtual InitResult addFrameBundle(const FrameBundle::Ptr& frames_cur) = 0;
  void setDepthPrior(double depth) { depth_at_current_frame_ = depth; have_depth_prior_ = true; }
  // R_cam_world of the frame the next addFrameBundle gets (initialization.h: setAbsoluteOrientationPrior)
  void setAbsoluteOrientationPrior(const svoh::Quat& R_cam_world) { R_cur_world_ = R_cam_world; have_rotation_prior_ = true; }
  void reset();
  bool have_depth_prior_ = false;
  double depth_at_current_frame_ = 1.0;
  bool have_rotation_prior_ = false;
  svoh::Quat R_ref_world_{ 1, 0, 0, 0 }, R_cur_world_{ 1, 0, 0, 0 };
  FrameBundle::Ptr frames_ref_;
  Transformation T_cur_from_ref_{ { 1, 0, 0, 0 }, { 0, 0, 0 } };
  // of the last addFrameBundle
  struct Statistics { size_t n_tracked = 0; double disparity = 0.0; size_t n_inliers = 0, n_triangulated = 0; double scale = 0.0, ms_ransac = 0.0; } stats_;
  FeatureTrackerHip& tracker() { return tracker_; }

 protected:
  // initialization.cpp:86-113: false = keep tracking (too few tracks: they are started again from this bundle, which becomes
  // the reference, R_ref_world_ = R_cur_world_; or too little disparity)
  bool trackFeaturesAndCheckDisparity(const FrameBundle::Ptr& frames);
  svoh_ctx* ctx_;
  InitializationOptions options_;
  FeatureTrackerHip tracker_;
};

// svo::HomographyInit (initialization.h, initialization.cpp:115-161) on one camera.
// Deviations: (1) the estimator (above); (2) a decomposition without four motions is a failure, not an abort; (3) kFailure
// resets the initialiser -- the caller goes on with the next frame, where processFirstFrame falls through to its keyframe
// code; (4) a failed triangulation restarts and returns kTracking, as the reference does.
class HomographyInitHip : public AbstractInitializationHip {
 public:
  HomographyInitHip(svoh_ctx* ctx, const InitializationOptions& init_options, const FeatureTrackerOptions& tracker_options,
                    const std::shared_ptr<DetectorHip>& detector);
  InitResult addFrameBundle(const FrameBundle::Ptr& frames_cur) override;
};

// svo::TwoPointInit (initialization.h, initialization.cpp:217-289) on one camera: the translation between the reference
// frame and the current one under the rotation the absolute orientation priors give (a gyroscope), then the triangulation.
// Without a prior set since the last call: kFailure before anything else (every call clears the flag).  Fewer inliers than
// init_min_inliers: kNoKeyframe.  A failed triangulation: kFailure.  Neither resets the initialiser; the caller goes on
// with the next frame, whose tracks are longer.
// Deviations: (1) the estimator -- opengv's RANSAC (100 iterations at most, probability 0.995) cannot be restated,
// svoh_translation_ransac_batch stands in its place with the reference's score; (2) its hypothesis count and seed are
// options (n_hypotheses, seed); (3) more than 1024 matches: std::runtime_error (the estimator's limit); (4) the threshold
// is computed at every call (the reference keeps the first call's in a function-level static).
class TwoPointInitHip : public AbstractInitializationHip {
 public:
  TwoPointInitHip(svoh_ctx* ctx, const InitializationOptions& init_options, const FeatureTrackerOptions& tracker_options,
                  const std::shared_ptr<DetectorHip>& detector);
  InitResult addFrameBundle(const FrameBundle::Ptr& frames_cur) override;
};

// svo::FivePointInit (initialization.h, initialization.cpp:292-359) on one camera: the relative pose between the reference
// frame and the current one from the matches alone, then the triangulation.  Too few tracks or too little disparity:
// kTracking.  Fewer inliers than init_min_inliers, or no model: kNoKeyframe.  A failed triangulation: kFailure.  Neither
// resets the initialiser; the caller goes on with the next frame, whose tracks are longer.
// Deviations: (1) the estimator -- opengv's RANSAC (100 iterations at most, probability 0.995) cannot be restated,
// svoh_essential_ransac_batch stands in its place with the score of the TwoPoint estimator; (2) its hypothesis count and
// seed are options (n_hypotheses, seed); (3) more than 1024 matches: std::runtime_error (the estimator's limit); (4) the
// threshold is computed at every call (the reference keeps the first call's in a function-level static).
class FivePointInitHip : public AbstractInitializationHip {
 public:
  FivePointInitHip(svoh_ctx* ctx, const InitializationOptions& init_options, const FeatureTrackerOptions& tracker_options,
                   const std::shared_ptr<DetectorHip>& detector);
  InitResult addFrameBundle(const FrameBundle::Ptr& frames_cur) override;
};

#endif  // SVOH_INIT_MATH_ONLY

}  // namespace svo_hip
