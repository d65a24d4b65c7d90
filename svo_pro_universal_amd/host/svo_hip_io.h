// svo_hip_io.h -- dataset / configuration plumbing for running the HIP front end on recorded
// sequences without OpenCV or yaml-cpp.  Counterparts in the reference:
//   examples/dataset/euroc.hpp:195-220      EuRoC folder layout, cam0/data.csv -> timestamps + image paths
//   examples/euroc_mono.cpp:11-62            the runner loop
//   src/svo/src/svo_factory.cpp:107-310      option keys and defaults read from the parameter YAML
//   examples/param/calib/*.yaml              NCamera calibration (vi::NCamera::loadFromYaml)
// Images: 8-bit PNG, grey or colour (colour is reduced like cv::imread + cv::cvtColor(BGR2GRAY),
// frame.cpp:72: fixed-point 0.299 R + 0.587 G + 0.114 B; identical to the input for grey files).
#pragma once

#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "svo_hip_host.h"
#include "svo_hip_init.h"

namespace svo_hip {
namespace io {

// ---- YAML subset: block maps, block sequences ("- key: v"), flow sequences "[a, b]" (may span
// lines), scalars, comments.  Enough for the reference's parameter and calibration files. ----
struct YamlNode {
  enum Kind { kNull, kScalar, kMap, kSeq } kind = kNull;
  std::string scalar;
  std::vector<std::pair<std::string, YamlNode>> map;   // insertion order kept
  std::vector<YamlNode> seq;
  bool has(const std::string& key) const;
  const YamlNode& operator[](const std::string& key) const;   // null node if absent (yaml-cpp style)
  const YamlNode& operator[](size_t i) const { return seq.at(i); }
  size_t size() const { return kind == kSeq ? seq.size() : map.size(); }
  bool isNull() const { return kind == kNull; }
  // node["key"].as<T>(fallback) of yaml-cpp
  double asDouble(double fallback) const;
  int asInt(int fallback) const;
  bool asBool(bool fallback) const;
  std::string asString(const std::string& fallback) const;
  std::vector<double> asDoubles() const;   // flow / block sequence of numbers
};
YamlNode parseYaml(const std::string& text);
YamlNode loadYamlFile(const std::string& path);

// ---- images ----
using GrayImage = svo_hip::GrayImage;   // (svo_hip_host.h)
GrayImage readPngGray(const std::string& path);                     // throws std::runtime_error
GrayImage decodePngGray(const uint8_t* bytes, size_t n_bytes);

// ---- camera rig ----
struct RigCamera {
  std::string label;
  svoh_camera cam{};
  Transformation T_B_C{ { 1, 0, 0, 0 }, { 0, 0, 0 } };   // body <- camera (T_imu_cam)
  // the camera's mask (camera_geometry_base.cpp:62-76): an 8-bit image of the camera's size, 0 = never a feature here; empty = none.
  // mask_file is the `mask:` key as the file has it; loadCameraRig reads the image, relative to the calibration file's directory.
  std::string mask_file;
  GrayImage mask;
  // the mask as a Frame carries it (Frame::mask), or null without one
  CameraMaskPtr maskPtr() const { return mask.data.empty() ? CameraMaskPtr() : std::make_shared<const GrayImage>(mask); }
};
// Both documents the reference loads: an NCamera (`cameras:` sequence, a `mask:` key inside a `camera:` node, ncamera.cpp:44-48)
// and a single camera (the camera's keys and `mask:` at the top level, camera_geometry_base.cpp:33-37; T_B_C = identity).
// A mask that cannot be read, or whose size is not the camera's, is an error ("Unable to load mask file", CHECK_EQ rows / cols).
std::vector<RigCamera> loadCameraRig(const std::string& calib_yaml_path);
// the same from a parsed document: without a directory to resolve `mask:` against, it records mask_file and leaves mask empty
std::vector<RigCamera> cameraRigFromYaml(const YamlNode& root);

// ---- the front-end options of svo_factory.cpp, for the parts this library implements ----
struct FrontendParams {
  SparseImgAlignOptions img_align;          // img_align_* (svo_factory.cpp:137-146)
  double img_align_prior_lambda_rot = 0.0, img_align_prior_lambda_trans = 0.0;
  int max_fts = 160;                         // reprojector: max_fts (svo_factory.cpp:207)
  int grid_size = 35;                        // grid_size
  double seed_sigma2_thresh = 200.0;         // seed_convergence_sigma2_thresh
  bool reprojector_affine_est_offset = true, reprojector_affine_est_gain = false;
  DepthFilterOptions depth_filter;           // depth filter keys (svo_factory.cpp:254-263)
  int max_n_seeds_per_frame = 360;           // max_fts * max_seeds_ratio
  DetectorOptions detector;                  // grid_size, n_pyr_levels, detector_threshold_*, use_edgelets
  FeatureTrackerOptions tracker;             // klt_* (svo_factory.cpp:305-306)
  int n_pyr_levels_to_build = 5;             // img_align_max_level + 1 (frame_handler_base.cpp:186)
  int structure_optimization_max_pts = 20;   // structure_optimization_max_pts (svo_factory.cpp:122)
  bool poseoptim_using_unit_sphere = false;  // pose optimiser on bearing-vector differences (frame_handler_base.cpp:137-138)
  // update_seeds_with_old_keyframes (svo_factory.cpp:147-148, default true): a new keyframe's seeds are updated with the last
  // frame and the overlap keyframes (frame_handler_mono.cpp:218-225).  Parsed only: the chains act on it where they are asked to
  // (svoh_mini_frontend: SVOH_MINI_SEEDS_OLD_KEYFRAMES; LockstepOptions::seeds_old_keyframes)
  bool update_seeds_with_old_keyframes = true;
  // the initialiser (svo_factory.cpp:178-195: init_min_features, init_min_tracked, init_min_inliers, init_min_disparity,
  // init_min_features_factor, reproj_err_thresh, init_disparity_pivot_ratio, init_method) and map_scale (:123), the depth prior
  // processFirstFrame hands it.  Parsed only: svoh_mini_frontend acts on them under SVOH_MINI_BOOTSTRAP.
  InitializationOptions init;
  double map_scale = 1.0;
};
FrontendParams frontendParamsFromYaml(const YamlNode& node);
FrontendParams loadFrontendParams(const std::string& param_yaml_path);

// ---- EuRoC ASL folder (<root>/mav0/cam0/data.csv, <root>/mav0/cam0/data/<timestamp>.png) ----
struct EurocSequence {
  std::string mav_dir;
  std::vector<uint64_t> cam_ts;             // nanoseconds
  std::vector<std::string> cam0_files, cam1_files;
  size_t size() const { return cam_ts.size(); }
};
EurocSequence openEuroc(const std::string& dataset_root);

// ---- EuRoC IMU (<root>/mav0/imu0/data.csv: "timestamp [ns], w_x, w_y, w_z [rad/s], a_x, a_y, a_z [m/s^2]") ----
struct ImuMeasurement { double t = 0.0; double w[3] = { 0, 0, 0 }; double a[3] = { 0, 0, 0 }; };   // t in seconds
std::vector<ImuMeasurement> readEurocImu(const std::string& dataset_root);   // ascending time; empty when the file is absent

// ImuHandler::getRelativeRotationPrior (src/svo/src/imu_handler.cpp:270-297 over getMeasurements, :157-233): the
// gyroscope integrated between two camera timestamps, R_oldimu_newimu = prod exp((omega_j - bias) dt_j) over the
// measurements from the newest one at or before t_old (its time moved to t_old) to the newest one before t_new (which
// counts up to t_new); camera times are shifted by delay_imu_cam first.  False (and identity) where the reference
// returns false: no measurement at or before t_old, none before t_new, both the same, or the newest one older than
// max_imu_delta_t.  `imu` in ascending time.
bool relativeRotationPrior(const std::vector<ImuMeasurement>& imu, double t_old_cam, double t_new_cam, const double gyro_bias[3],
                           double delay_imu_cam, double max_imu_delta_t, svoh::Quat* R_oldimu_newimu);

// ---- trajectory output, TUM format: "timestamp tx ty tz qx qy qz qw" (seconds) ----
class TrajectoryWriter {
 public:
  explicit TrajectoryWriter(const std::string& path);
  ~TrajectoryWriter();
  void write(uint64_t timestamp_ns, const Transformation& T_world_body);
 private:
  struct Impl;
  std::unique_ptr<Impl> impl_;
};

}  // namespace io
}  // namespace svo_hip
