// mask_tool.cpp -- the calibration loader's camera masks, for tests/test_camera_masks_cpu.py.  No GPU call.
//   mask_tool rig <calib.yaml>        per camera: "camera <label> <width> <height>", "mask_file <name|->",
//                                     "mask <width> <height> <zero pixels> <sum of all pixels>" (0 0 0 0 without a mask)
// An exception: "error <text>", exit status 1.
#include <cstdio>
#include <string>
#include <vector>

#include "../../svo_pro_universal_amd/host/svo_hip_io.h"

using namespace svo_hip;

int main(int argc, char** argv)
{
  if (argc != 3) return 2;
  const std::string what = argv[1];
  try {
    if (what != "rig") return 2;
    const std::vector<io::RigCamera> rig = io::loadCameraRig(argv[2]);
    for (const io::RigCamera& c : rig) {
      size_t zeros = 0;
      unsigned long long sum = 0;
      for (uint8_t v : c.mask.data) { zeros += v == 0; sum += v; }
      printf("camera %s %d %d\nmask_file %s\nmask %d %d %zu %llu\n", c.label.c_str(), c.cam.width, c.cam.height, c.mask_file.empty() ? "-" : c.mask_file.c_str(),
             c.mask.width, c.mask.height, zeros, sum);
    }
  } catch (const std::exception& e) {
    printf("error %s\n", e.what());
    return 1;
  }
  return 0;
}
