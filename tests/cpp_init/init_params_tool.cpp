// init_params_tool <params.yaml|->: prints the initialiser's options and map_scale as svo_hip::io::loadFrontendParams reads
// them ("-": an empty document, every key absent).  Driven by tests/test_init_params_cpu.py; no GPU call.
#include <cstdio>
#include <exception>
#include <string>

#include "../../svo_pro_universal_amd/host/svo_hip_io.h"

int main(int argc, char** argv)
{
  if (argc != 2) { fprintf(stderr, "usage: %s <params.yaml|->\n", argv[0]); return 2; }
  try {
    using namespace svo_hip;
    const io::FrontendParams p = std::string(argv[1]) == "-" ? io::frontendParamsFromYaml(io::YamlNode()) : io::loadFrontendParams(argv[1]);
    printf("init_min_features=%zu\ninit_min_tracked=%zu\ninit_min_inliers=%zu\n", p.init.init_min_features, p.init.init_min_tracked, p.init.init_min_inliers);
    printf("init_min_disparity=%.17g\ninit_min_features_factor=%.17g\ninit_disparity_pivot_ratio=%.17g\n", p.init.init_min_disparity, p.init.init_min_features_factor,
           p.init.init_disparity_pivot_ratio);
    printf("reproj_err_thresh=%.17g\nmap_scale=%.17g\ninit_method=%s\ninit_type=%d\n", p.init.reproj_error_thresh, p.map_scale, p.init.init_method.c_str(), (int)p.init.init_type);
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "init_params_tool: %s\n", e.what());
    return 1;
  }
}
