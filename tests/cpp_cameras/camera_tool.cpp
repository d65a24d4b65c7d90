// camera_tool.cpp -- host side of the wide camera models, for tests/test_camera_models_cpu.py.  No GPU call.
//   camera_tool params <param.yaml>        the front-end keys the camera models bring (poseoptim_using_unit_sphere, ...)
//   camera_tool maths <calib.yaml> <in> <out>
//       in: n x 3 doubles (points in the camera frame); out: n x 11 doubles per point: px (2), J (6, row-major; NaN for
//       ATAN, which has none), back-projection of px (3) -- svoh_math.h's CamModelWide as g++ compiles it (libm)
//   camera_tool host <calib.yaml> <in> <out>
//       the host layer's own camera sites on a Frame with that camera (T_f_w = identity): per point px (2) and
//       visibility (1) of Frame::isVisible, then the bearing vector (3) depth_filter_utils::appendSeeds gives the
//       feature at px (computeNormalizedBearingVectors)
#include <cmath>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "../../svo_pro_universal_amd/host/svo_hip_host.h"
#include "../../svo_pro_universal_amd/host/svo_hip_io.h"
#include "../../svo_pro_universal_amd/csrc/svoh_math.h"

using namespace svo_hip;

int main(int argc, char** argv)
{
  if (argc < 3) return 2;
  const std::string what = argv[1];
  try {
    if (what == "params") {
      const io::FrontendParams p = io::loadFrontendParams(argv[2]);
      printf("poseoptim_using_unit_sphere %d\nuse_distortion_jacobian %d\nscan_epi_unit_sphere %d\n", (int)p.poseoptim_using_unit_sphere,
             (int)p.img_align.use_distortion_jacobian, (int)p.depth_filter.scan_epi_unit_sphere);
    } else if (what == "maths" && argc == 5) {
      const std::vector<io::RigCamera> rig = io::loadCameraRig(argv[2]);
      const svoh::CamModelWide cm = svoh::load_camera_wide(rig.at(0).cam);
      FILE* f = fopen(argv[3], "rb");
      if (!f) return 3;
      std::vector<double> in;
      double v[3];
      while (fread(v, sizeof(double), 3, f) == 3) in.insert(in.end(), v, v + 3);
      fclose(f);
      std::vector<double> out;
      for (size_t i = 0; i + 2 < in.size(); i += 3) {
        const svoh::Vec3 p = { in[i], in[i + 1], in[i + 2] };
        double u, w, J[6];
        svoh::project3(cm, p, u, w);
        if (svoh::camera_has_jacobian(rig[0].cam)) svoh::project3_jacobian(cm, p, J);
        else for (double& j : J) j = NAN;
        const svoh::Vec3 b = svoh::back_project3(cm, u, w);
        const double row[11] = { u, w, J[0], J[1], J[2], J[3], J[4], J[5], b.x, b.y, b.z };
        out.insert(out.end(), row, row + 11);
      }
      f = fopen(argv[4], "wb");
      if (!f) return 3;
      fwrite(out.data(), sizeof(double), out.size(), f);
      fclose(f);
      printf("n %zu\n", out.size() / 11);
    } else if (what == "host" && argc == 5) {
      const std::vector<io::RigCamera> rig = io::loadCameraRig(argv[2]);
      auto frame = std::make_shared<Frame>();
      frame->cam = rig.at(0).cam;
      FILE* f = fopen(argv[3], "rb");
      if (!f) return 3;
      std::vector<double> in;
      double v[3];
      while (fread(v, sizeof(double), 3, f) == 3) in.insert(in.end(), v, v + 3);
      fclose(f);
      const size_t n = in.size() / 3;
      std::vector<double> px(2 * n), vis(n);
      for (size_t i = 0; i < n; ++i) {
        const svoh::Vec3 p = { in[3 * i], in[3 * i + 1], in[3 * i + 2] };
        vis[i] = frame->isVisible(p, &px[2 * i]) ? 1.0 : 0.0;
      }
      depth_filter_utils::appendSeeds(frame, px, std::vector<double>(n, 0.0), std::vector<int32_t>(n, 0), std::vector<double>(2 * n, 0.0),
                                      std::vector<uint8_t>(n, SVOH_FT_CORNER), 1.0f, 2.0f);
      std::vector<double> out;
      for (size_t i = 0; i < n; ++i) {
        const double row[6] = { px[2 * i], px[2 * i + 1], vis[i], frame->f_vec_[3 * i], frame->f_vec_[3 * i + 1], frame->f_vec_[3 * i + 2] };
        out.insert(out.end(), row, row + 6);
      }
      f = fopen(argv[4], "wb");
      if (!f) return 3;
      fwrite(out.data(), sizeof(double), out.size(), f);
      fclose(f);
      printf("n %zu\n", n);
    } else {
      return 2;
    }
  } catch (const std::exception& e) {
    printf("error %s\n", e.what());
    return 1;
  }
  return 0;
}
