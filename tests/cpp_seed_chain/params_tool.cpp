// params_tool <params.yaml|->: prints "update_seeds_with_old_keyframes=<0|1>" as svo_hip::io::loadFrontendParams reads it
// ("-": an empty document, every key absent).  Driven by tests/test_seed_chain_cpu.py; no GPU call.
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
    printf("update_seeds_with_old_keyframes=%d\n", p.update_seeds_with_old_keyframes ? 1 : 0);
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "params_tool: %s\n", e.what());
    return 1;
  }
}
