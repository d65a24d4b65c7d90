// init_tool -- the host maths of the mono bootstrap (svo_hip_init.h, the part that makes no device call) on a case read
// from a text file; prints what tests/test_init_cpu.py compares with tests/np_restatement_init.py.
//   init_tool <case file>
// Case file, one item per line:  H <9>  |  thresh <t>  |  depth <d>  |  angle <a>  |  pivot <r>  |  focal <f>  |  px <reproj px>
//   T_ref_world <qw qx qy qz tx ty tz>  |  match <f_cur 3> <f_ref 3> <inlier 0/1>  |  ids1 <...>  |  ids2 <...>  |  disp <...>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../svo_pro_universal_amd/host/svo_hip_init.h"

using namespace svo_hip;

static void print_vec(const char* key, const double* v, size_t n)
{
  printf("%s", key);
  for (size_t i = 0; i < n; ++i) printf(" %.17g", v[i]);
  printf("\n");
}

int main(int argc, char** argv)
{
  if (argc != 2) { fprintf(stderr, "usage: %s <case file>\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  if (!in) { fprintf(stderr, "init_tool: cannot read %s\n", argv[1]); return 2; }
  double H[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 }, thresh = 0.005, depth = 1.0, angle = 0.005, pivot = 0.5, focal = 400.0, px = 2.0;
  svoh::Rigid T_ref_world{ { 1, 0, 0, 0 }, { 0, 0, 0 } };
  std::vector<double> f_cur, f_ref, disp;
  std::vector<uint8_t> inl;
  std::vector<int> ids1, ids2;
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string key;
    if (!(ss >> key)) continue;
    std::vector<double> v;
    std::string tok;
    while (ss >> tok) v.push_back(strtod(tok.c_str(), nullptr));   // strtod reads "nan" and "inf"
    auto need = [&](size_t k) { if (v.size() != k) throw std::runtime_error("init_tool: bad line: " + line); };
    try {
      if (key == "H") { need(9); for (int i = 0; i < 9; ++i) H[i] = v[(size_t)i]; }
      else if (key == "thresh") { need(1); thresh = v[0]; }
      else if (key == "depth") { need(1); depth = v[0]; }
      else if (key == "angle") { need(1); angle = v[0]; }
      else if (key == "pivot") { need(1); pivot = v[0]; }
      else if (key == "focal") { need(1); focal = v[0]; }
      else if (key == "px") { need(1); px = v[0]; }
      else if (key == "T_ref_world") { need(7); T_ref_world = svoh::Rigid{ { v[0], v[1], v[2], v[3] }, { v[4], v[5], v[6] } }; }
      else if (key == "match") { need(7); f_cur.insert(f_cur.end(), v.begin(), v.begin() + 3); f_ref.insert(f_ref.end(), v.begin() + 3, v.begin() + 6); inl.push_back(v[6] != 0.0); }
      else if (key == "ids1") for (double x : v) ids1.push_back((int)x);
      else if (key == "ids2") for (double x : v) ids2.push_back((int)x);
      else if (key == "disp") disp = v;
      else throw std::runtime_error("init_tool: unknown key " + key);
    } catch (const std::exception& e) { fprintf(stderr, "%s\n", e.what()); return 2; }
  }
  const size_t n = inl.size();
  double sv[3];
  vk::singularValues3(H, sv);
  print_vec("singular_values", sv, 3);
  std::vector<vk::CameraMotion> motions;
  vk::decomposeHomography(H, &motions);
  printf("n_motions %zu\n", motions.size());
  for (const vk::CameraMotion& m : motions) { print_vec("motion_R", m.R, 9); print_vec("motion_t", m.t, 3); print_vec("motion_n", m.n, 3); }
  double cheir[4];
  int picked = -1;
  const vk::Homography sel = vk::selectMotion(H, f_cur.data(), f_ref.data(), inl.data(), n, thresh, cheir, &picked);
  print_vec("cheirality", cheir, 4);
  printf("picked %d\n", picked);
  printf("score %.17g\n", sel.score);
  print_vec("selected_R", sel.R_cur_ref, 9);
  print_vec("selected_t", sel.t_cur_ref, 3);
  print_vec("selected_n", sel.n_cur, 3);
  if (sel.score > 0) {
    const svoh::Rigid T_cur_ref{ vk::quaternionFromRotation(sel.R_cur_ref), { sel.t_cur_ref[0], sel.t_cur_ref[1], sel.t_cur_ref[2] } };
    initialization_utils::FeatureMatches matches;
    for (size_t i = 0; i < n; ++i) matches.emplace_back(i, i);
    std::vector<double> pts;
    initialization_utils::triangulatePoints(f_cur.data(), f_ref.data(), T_cur_ref, angle, true, &matches, &pts);
    printf("triangulated");
    for (const auto& m : matches) printf(" %zu", m.first);
    printf("\n");
    print_vec("points_in_cur", pts.data(), pts.size());
    try {
      double scale = 0;
      svoh::Rigid T_cur_world;
      std::vector<double> world;
      initialization_utils::rescalePoints(pts, T_cur_ref, T_ref_world, depth, &scale, &T_cur_world, &world);
      printf("scale %.17g\n", scale);
      const double T[7] = { T_cur_world.q.w, T_cur_world.q.x, T_cur_world.q.y, T_cur_world.q.z, T_cur_world.t.x, T_cur_world.t.y, T_cur_world.t.z };
      print_vec("T_cur_world", T, 7);
      print_vec("points_in_world", world.data(), world.size());
    } catch (const std::exception& e) { printf("rescale_refused %s\n", e.what()); }
    std::vector<double> xyz;
    std::vector<int> inliers, outliers;
    vk::computeInliers(f_cur.data(), f_ref.data(), n, sel.R_cur_ref, sel.t_cur_ref, px, focal, &xyz, &inliers, &outliers);
    printf("compute_inliers");
    for (int i : inliers) printf(" %d", i);
    printf("\n");
  }
  printf("disparity_percentile %.17g\n", feature_tracking_utils::getTracksDisparityPercentile(disp, pivot));
  std::vector<std::pair<size_t, size_t>> m12;
  feature_tracking_utils::getFeatureMatches(ids1.data(), ids1.size(), ids2.data(), ids2.size(), &m12);
  printf("feature_matches");
  for (const auto& m : m12) printf(" %zu:%zu", m.first, m.second);
  printf("\n");
  return 0;
}
