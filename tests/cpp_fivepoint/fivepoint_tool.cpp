// fivepoint_tool -- the essential-matrix estimator of include/svo_hip.h (svoh_essential_ransac_batch) run serially on the
// CPU with the very functions the kernel runs (csrc/svoh_essential.h), on a case read from a text file; prints what
// tests/test_fivepoint_cpu.py compares with tests/np_restatement_fivepoint.py.  No device call, nothing linked.
//   fivepoint_tool <case file>
// Case file, one item per line:  K <hypotheses>  |  thresh <t>  |  seed <64-bit>  |  match <f_cur 3> <f_ref 3>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../svo_pro_universal_amd/csrc/svoh_essential.h"

using namespace svoh;

int main(int argc, char** argv)
{
  if (argc != 2) { fprintf(stderr, "usage: %s <case file>\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  if (!in) { fprintf(stderr, "fivepoint_tool: cannot read %s\n", argv[1]); return 2; }
  double thresh = 1e-5;
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
    else if (key == "match" && tok.size() == 6) for (size_t i = 0; i < 3; ++i) { f_cur.push_back(num(i)); f_ref.push_back(num(3 + i)); }
    else ok = false;
    if (!ok) { fprintf(stderr, "fivepoint_tool: bad line: %s\n", line.c_str()); return 2; }
  }
  const int n = (int)(f_cur.size() / 3);
  const int cap = n > 0 ? n : 1;
  std::vector<double> cols((size_t)kEssentialCols * (size_t)cap, 0.0);
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) {
      cols[(size_t)k * (size_t)cap + (size_t)i] = f_cur[3 * (size_t)i + (size_t)k];
      cols[(size_t)(3 + k) * (size_t)cap + (size_t)i] = f_ref[3 * (size_t)i + (size_t)k];
    }

  long best_h = -1, n_degenerate = 0, n_models = 0, n_hold_all = 0;   // n_hold_all: hypotheses whose best candidate holds every match
  int best_count = -1, best_c = 0;
  double R0[9] = { 0 }, t0[3] = { 0 };
  if (n >= 5) {
    for (long h = 0; h < K; ++h) {
      int models, count, candidate;
      double R[9], t[3];
      if (!essential_hypothesis(seed, (unsigned)h, cols.data(), cap, n, thresh, models, count, candidate, R, t)) { ++n_degenerate; continue; }
      n_models += models;
      if (models > 0 && count == n) ++n_hold_all;
      if (models > 0 && count > best_count) {
        best_count = count; best_h = h; best_c = candidate;
        for (int k = 0; k < 9; ++k) R0[k] = R[k];
        for (int k = 0; k < 3; ++k) t0[k] = t[k];
      }
    }
  }
  std::vector<int> mask((size_t)n, 0);
  auto print9 = [](const char* name, const double* v, int m) { printf("%s", name); for (int k = 0; k < m; ++k) printf(" %.17g", v[k]); printf("\n"); };
  if (best_h < 0 || best_count < 5) {
    const double zero[9] = { 0 };
    printf("status 1\nbest_hypothesis 0\nbest_candidate 0\nn_inliers_hypothesis 0\nn_inliers 0\nn_degenerate 0\nn_models 0\nrefine_iters 0\n");
    print9("R", zero, 9); print9("t", zero, 3); print9("R_winner", zero, 9); print9("t_winner", zero, 3);
  } else {
    std::vector<int> inl;
    for (int i = 0; i < n; ++i) if (essential_is_inlier(R0, t0, cols.data(), cap, i, thresh)) inl.push_back(i);
    double R[9], t[3];
    for (int k = 0; k < 9; ++k) R[k] = R0[k];
    for (int k = 0; k < 3; ++k) t[k] = t0[k];
    int iters = 0;
    for (int iter = 0; iter < 10; ++iter) {
      double b1[3], b2[3], acc[kEssentialNAcc] = { 0 };
      essential_tangent(t, b1, b2);
      for (int i : inl) essential_accumulate(R, t, b1, b2, cols.data(), cap, i, acc);
      double m[25], d[5], tmp[5];
      int tr[5];
      for (int r = 0; r < 5; ++r)
        for (int c = 0; c < 5; ++c) m[c * 5 + r] = r >= c ? acc[r * (r + 1) / 2 + c] : acc[c * (c + 1) / 2 + r];
      for (int k = 0; k < 5; ++k) d[k] = acc[15 + k];
      ldlt_solve_inplace<5>(m, d, tr, tmp);
      iters = iter + 1;
      bool finite = true;
      double biggest = 0.0;
      for (int k = 0; k < 5; ++k) { finite = finite && tr_finite(d[k]); biggest = fmax(biggest, fabs(d[k])); }
      if (!finite) break;
      essential_update(d, b1, b2, R, t);
      if (biggest < 1e-10) break;
    }
    int n_inliers = 0;
    for (int i = 0; i < n; ++i) { mask[(size_t)i] = essential_is_inlier(R, t, cols.data(), cap, i, thresh) ? 1 : 0; n_inliers += mask[(size_t)i]; }
    printf("status 0\nbest_hypothesis %ld\nbest_candidate %d\nn_inliers_hypothesis %d\nn_inliers %d\nn_degenerate %ld\nn_models %ld\nrefine_iters %d\n",
           best_h, best_c, best_count, n_inliers, n_degenerate, n_models, iters);
    print9("R", R, 9); print9("t", t, 3); print9("R_winner", R0, 9); print9("t_winner", t0, 3);
  }
  printf("n_hold_all %ld\n", n_hold_all);
  printf("mask");
  for (int i = 0; i < n; ++i) printf(" %d", mask[(size_t)i]);
  printf("\n");
  return 0;
}
