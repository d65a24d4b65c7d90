// twopoint_tool -- the translation estimator of include/svo_hip.h (svoh_translation_ransac_batch) run serially on the
// CPU with the very functions the kernel runs (csrc/svoh_translation.h), on a case read from a text file; prints what
// tests/test_twopoint_cpu.py compares with tests/np_restatement_twopoint.py.  No device call, nothing linked.
//   twopoint_tool <case file>
// Case file, one item per line:  K <hypotheses>  |  thresh <t>  |  seed <64-bit>  |  R <9, row-major>  |  match <f_cur 3> <f_ref 3>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../svo_pro_universal_amd/csrc/svoh_translation.h"

using namespace svoh;

int main(int argc, char** argv)
{
  if (argc != 2) { fprintf(stderr, "usage: %s <case file>\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  if (!in) { fprintf(stderr, "twopoint_tool: cannot read %s\n", argv[1]); return 2; }
  double R[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 }, thresh = 1e-5;
  unsigned long long seed = 0;
  long K = 2000;
  std::vector<double> f_cur, f_ref;
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string key;
    if (!(ss >> key)) continue;
    std::vector<std::string> tok;
    std::string s;
    while (ss >> s) tok.push_back(s);
    auto num = [&](size_t i) { return strtod(tok[i].c_str(), nullptr); };   // strtod reads "nan" and "inf"
    bool ok = true;
    if (key == "K" && tok.size() == 1) K = atol(tok[0].c_str());
    else if (key == "thresh" && tok.size() == 1) thresh = num(0);
    else if (key == "seed" && tok.size() == 1) seed = strtoull(tok[0].c_str(), nullptr, 10);
    else if (key == "R" && tok.size() == 9) for (size_t i = 0; i < 9; ++i) R[i] = num(i);
    else if (key == "match" && tok.size() == 6) for (size_t i = 0; i < 3; ++i) { f_cur.push_back(num(i)); f_ref.push_back(num(3 + i)); }
    else ok = false;
    if (!ok) { fprintf(stderr, "twopoint_tool: bad line: %s\n", line.c_str()); return 2; }
  }
  const int n = (int)(f_cur.size() / 3);
  const int cap = n > 0 ? n : 1;
  std::vector<double> cols((size_t)kTranslationCols * (size_t)cap, 0.0);
  for (int i = 0; i < n; ++i) {
    double col[kTranslationCols];
    translation_stage(R, &f_cur[3 * (size_t)i], &f_ref[3 * (size_t)i], col);
    for (int k = 0; k < kTranslationCols; ++k) cols[(size_t)k * (size_t)cap + (size_t)i] = col[k];
  }
  auto column3 = [&](int first, unsigned i, double out[3]) { for (int k = 0; k < 3; ++k) out[k] = cols[(size_t)(first + k) * (size_t)cap + i]; };

  long best_h = -1, n_degenerate = 0;
  int best_count = -1;
  double best_t[3] = { 0, 0, 0 };
  if (n >= 2) {
    for (long h = 0; h < K; ++h) {
      unsigned i, j;
      double t[3];
      bool ok = translation_sample(seed, (unsigned)h, (unsigned)n, i, j);
      if (ok) {
        double fi[3], gi[3], fj[3], gj[3];
        column3(0, i, fi); column3(3, i, gi); column3(0, j, fj); column3(3, j, gj);
        ok = translation_from_two(fi, gi, fj, gj, t);
      }
      if (!ok) { ++n_degenerate; continue; }
      const int count = translation_count_inliers(t, cols.data(), cap, n, thresh);
      if (count > best_count) { best_count = count; best_h = h; best_t[0] = t[0]; best_t[1] = t[1]; best_t[2] = t[2]; }
    }
  }
  std::vector<int> mask((size_t)n, 0);
  if (best_h < 0 || best_count < 2) {
    printf("status 1\nbest_hypothesis 0\nn_inliers_hypothesis 0\nn_inliers 0\nn_degenerate 0\nt 0 0 0\nt_winner 0 0 0\n");
  } else {
    double M[6] = { 0, 0, 0, 0, 0, 0 }, t[3];
    for (int i = 0; i < n; ++i)
      if (translation_is_inlier(best_t, cols.data(), cap, i, thresh)) translation_accumulate(cols.data(), cap, i, M);
    translation_refine(M, best_t, t);
    int n_inliers = 0;
    for (int i = 0; i < n; ++i) { mask[(size_t)i] = translation_is_inlier(t, cols.data(), cap, i, thresh) ? 1 : 0; n_inliers += mask[(size_t)i]; }
    printf("status 0\nbest_hypothesis %ld\nn_inliers_hypothesis %d\nn_inliers %d\nn_degenerate %ld\n", best_h, best_count, n_inliers, n_degenerate);
    printf("t %.17g %.17g %.17g\n", t[0], t[1], t[2]);
    printf("t_winner %.17g %.17g %.17g\n", best_t[0], best_t[1], best_t[2]);
  }
  printf("mask");
  for (int i = 0; i < n; ++i) printf(" %d", mask[(size_t)i]);
  printf("\n");
  return 0;
}
