// test_host_align_wide.cpp -- SparseImgAlignHip on a bundle with an EQUIDISTANT or ATAN camera: the blocking overload
// run(ref, cur) goes through svoh_sparse_align_wide_batch and leaves the frame poses
//     T_f_w = T_cam_imu * T_icur_iref * T_iref_world      (sparse_img_align.cpp:103-106)
// of that entry's result; the after_enqueue overload and runSplit throw.
// Input: a scene dump written by tests/test_host_cpp_wide_gpu.py.  Exit code 0 = pass.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../svo_pro_universal_amd/host/svo_hip_host.h"

using namespace svo_hip;

static std::vector<double> read_doubles(FILE* f, size_t n)
{
  std::vector<double> v(n);
  if (fread(v.data(), sizeof(double), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
  return v;
}

static Transformation to_T(const double* v) { Transformation T{ { v[0], v[1], v[2], v[3] }, { v[4], v[5], v[6] } }; return T; }

#define CHECK(cond)                                                            \
  do { if (!(cond)) { fprintf(stderr, "CHECK failed: %s (%s:%d)\n", #cond, __FILE__, __LINE__); return 1; } } while (0)

int main(int argc, char** argv)
{
  if (argc < 2) { fprintf(stderr, "usage: %s scene.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror("open"); return 2; }
  int32_t hdr[4];  // width, height, n_features, distortion (svoh_distortion)
  CHECK(fread(hdr, sizeof(int32_t), 4, f) == 4);
  const int w = hdr[0], h = hdr[1], n = hdr[2];
  std::vector<double> camv = read_doubles(f, 8);  // fx fy cx cy d0 d1 d2 d3
  std::vector<double> T_cam_imu = read_doubles(f, 7), T_ref_f_w = read_doubles(f, 7), T_cur_init_f_w = read_doubles(f, 7);
  std::vector<double> px = read_doubles(f, 2 * (size_t)n), fv = read_doubles(f, 3 * (size_t)n), pw = read_doubles(f, 3 * (size_t)n);
  std::vector<uint8_t> flags(n), img_ref((size_t)w * h), img_cur((size_t)w * h);
  CHECK(fread(flags.data(), 1, n, f) == (size_t)n);
  CHECK(fread(img_ref.data(), 1, img_ref.size(), f) == img_ref.size());
  CHECK(fread(img_cur.data(), 1, img_cur.size(), f) == img_cur.size());
  fclose(f);

  svoh_ctx* ctx = nullptr;
  if (svoh_create(0, &ctx) != SVOH_OK) { fprintf(stderr, "svoh_create: %s\n", svoh_last_error_string(nullptr)); return 3; }

  svoh_camera cam{};
  cam.fx = camv[0]; cam.fy = camv[1]; cam.cx = camv[2]; cam.cy = camv[3];
  for (int i = 0; i < 4; ++i) cam.d[i] = camv[4 + i];
  cam.distortion = hdr[3];
  cam.width = w; cam.height = h;
  CHECK(cam.distortion == SVOH_DISTORTION_EQUIDISTANT || cam.distortion == SVOH_DISTORTION_ATAN);

  const int n_levels = 5;
  FramePtr ref(new Frame), cur(new Frame);
  CHECK(svoh_build_pyramid(ctx, img_ref.data(), w, h, w, SVOH_MEM_HOST, n_levels, SVOH_HALFSAMPLE_REFERENCE, nullptr, &ref->pyramid) == SVOH_OK);
  CHECK(svoh_build_pyramid(ctx, img_cur.data(), w, h, w, SVOH_MEM_HOST, n_levels, SVOH_HALFSAMPLE_REFERENCE, nullptr, &cur->pyramid) == SVOH_OK);
  ref->cam = cam; cur->cam = cam;
  ref->set_T_cam_imu(to_T(T_cam_imu.data())); cur->set_T_cam_imu(to_T(T_cam_imu.data()));
  ref->T_f_w_ = to_T(T_ref_f_w.data());
  cur->T_f_w_ = to_T(T_cur_init_f_w.data());
  ref->num_features_ = (size_t)n;
  ref->px_vec_ = px; ref->f_vec_ = fv; ref->pos_world_ = pw; ref->alignable_ = flags;

  FrameBundle::Ptr last_frames(new FrameBundle), new_frames(new FrameBundle);
  last_frames->frames_.push_back(ref);
  new_frames->frames_.push_back(cur);

  SparseImgAlignOptions img_align_options;
  img_align_options.max_level = 4;
  img_align_options.min_level = 2;  // svo_factory.cpp:137-138
  SparseImgAlignHip align(ctx, SparseImgAlignHip::getDefaultSolverOptions(), img_align_options);
  align.reset();
  const Transformation T_iref_world = ref->T_imu_world();
  const Transformation T_icur_iref_init = svoh::mul(cur->T_imu_world(), svoh::inverse(T_iref_world));

  // ---- the C entry on the same problem ----
  svoh_align_options opt{};
  opt.max_level = 4; opt.min_level = 2; opt.patch_size = 4; opt.max_iter = 10; opt.eps = 0.0005; opt.weight_scale = 10;
  svoh_align_problem pb{};
  pb.n_cams = 1;
  svoh_align_camera& pc = pb.cams[0];
  pc.ref_frame = ref->pyramid; pc.cur_frame = cur->pyramid; pc.cam = cam;
  svoh::store_rigid(ref->T_imu_cam(), pc.ref_T_imu_cam);
  svoh::store_rigid(ref->T_cam_imu(), pc.ref_T_cam_imu);
  svoh::store_rigid(cur->T_cam_imu(), pc.cur_T_cam_imu);
  const svoh::Vec3 rp = ref->pos();
  pc.ref_pos[0] = rp.x; pc.ref_pos[1] = rp.y; pc.ref_pos[2] = rp.z;
  pc.n_features = n; pc.mem_space = SVOH_MEM_HOST;
  pc.px = px.data(); pc.f = fv.data(); pc.pos_world = pw.data(); pc.flags = flags.data();
  svoh::store_rigid(T_icur_iref_init, pb.T_icur_iref);
  svoh_align_result cres{};
  CHECK(svoh_sparse_align_wide_batch(ctx, &opt, 1, &pb, &cres) == SVOH_OK);
  CHECK(cres.status == 0 && cres.n_fts_to_track > 0);
  svoh_align_result narrow{};
  CHECK(svoh_sparse_align_batch(ctx, &opt, 1, &pb, &narrow) == SVOH_ERR_INVALID_ARGUMENT);   // the narrow entry goes on refusing

  // ---- the mirror: the blocking overload ----
  const size_t n_tracked = align.run(last_frames, new_frames);
  CHECK((int)n_tracked == cres.n_fts_to_track);
  for (int l = 0; l < SVOH_MAX_LEVELS; ++l) CHECK(align.lastResult().iters[l] == cres.iters[l]);
  const Transformation T_exp = svoh::mul(svoh::mul(cur->T_cam_imu(), svoh::load_rigid(cres.T_icur_iref)), T_iref_world);
  const double d[7] = { cur->T_f_w_.q.w - T_exp.q.w, cur->T_f_w_.q.x - T_exp.q.x, cur->T_f_w_.q.y - T_exp.q.y,
                        cur->T_f_w_.q.z - T_exp.q.z, cur->T_f_w_.t.x - T_exp.t.x, cur->T_f_w_.t.y - T_exp.t.y,
                        cur->T_f_w_.t.z - T_exp.t.z };
  double m = 0;
  for (double v : d) m = fmax(m, fabs(v));
  const Transformation T_start = to_T(T_cur_init_f_w.data());
  const double moved = fmax(fabs(cur->T_f_w_.t.x - T_start.t.x), fmax(fabs(cur->T_f_w_.t.y - T_start.t.y), fabs(cur->T_f_w_.t.z - T_start.t.z)));
  printf("tracked %zu, |T_f_w(run) - T_cam_imu T_icur_iref T_iref_world| = %.3e, moved %.3e\n", n_tracked, m, moved);
  CHECK(m == 0.0);       // one kernel, one geometry, the same composition: the same bits
  CHECK(moved > 1e-4);   // the alignment did something

  // ---- the overloads that queue ----
  cur->T_f_w_ = T_start;
  bool threw = false, hook_ran = false;
  std::string what;
  try { align.run(last_frames, new_frames, [&](const Transformation&) { hook_ran = true; }); }
  catch (const std::runtime_error& e) { threw = true; what = e.what(); }
  CHECK(threw && !hook_ran && what.find("blocking overload") != std::string::npos);
  threw = false;
  try { align.runSplit(last_frames, new_frames, 0, 1, nullptr); } catch (const std::runtime_error& e) { threw = true; what = e.what(); }
  CHECK(threw && what.find("blocking overload") != std::string::npos);
  CHECK(cur->T_f_w_.t.x == T_start.t.x && cur->T_f_w_.q.w == T_start.q.w);   // neither touched the frame

  svoh_destroy(ctx);
  printf("PASS\n");
  return 0;
}
