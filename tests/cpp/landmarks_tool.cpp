// The landmark bookkeeping of the host mirrors on a script of events, for the comparison with the independent reading in
// tests/landmark_cases.py (which documents the script and the dump): upgradeSeedsToFeatures, StereoTriangulationHip::finish with
// the script's match arrays and a fixed Job, initialization_utils::rescaleAndInitializePoints, removeObservationsOf,
// Point::addObservation and StructureBatch::gather / apply.
//   landmarks_tool <script.txt> <dump.txt> [--device]
// Without --device no device call is made: a structure step is optimizeStructure's loop with gather's output written out in
// place of the kernel's launch, and the positions the script supplies applied.  With --device a context is created and a
// structure step is optimizeStructure(ctx, bundle, max_n_pts, 5) itself.
// A std::runtime_error from a mirror ends the script: "throw <event>" goes to the dump, the message to stderr, the state follows.
#include <algorithm>
#include <cstdio>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../svo_pro_universal_amd/host/svo_hip_host.h"
#include "../../svo_pro_universal_amd/host/svo_hip_init.h"
using namespace svo_hip;

namespace {
struct Scene {
  std::map<int, FramePtr> held;                 // the scene's own pointers
  std::map<int, std::weak_ptr<Frame>> frames;   // every frame ever made
  std::map<int, PointPtr> registered;           // the script's own points
  FILE* out = nullptr;

  FramePtr frame(int id) const
  {
    auto it = frames.find(id);
    FramePtr f = it == frames.end() ? nullptr : it->second.lock();
    if (!f) throw std::logic_error("script: no live frame " + std::to_string(id));
    return f;
  }
  void state() const
  {
    std::map<int, PointPtr> shown(registered);
    for (const auto& kv : frames)
      if (const FramePtr f = kv.second.lock())
        for (size_t i = 0; i < f->num_features_; ++i)
          if (f->landmark_vec_[i]) shown[f->landmark_vec_[i]->id()] = f->landmark_vec_[i];
    fprintf(out, "state\n");
    for (const auto& kv : shown) {
      const Point& p = *kv.second;
      std::string obs;
      int n_live = 0;
      for (const Point::Obs& o : p.obs_)
        if (const FramePtr f = o.frame.lock()) { obs += " " + std::to_string(f->id()) + " " + std::to_string(o.keypoint_index_); ++n_live; }
      fprintf(out, "point %d %.17g %.17g %.17g %d %d%s\n", p.id(), p.pos_.x, p.pos_.y, p.pos_.z, p.last_structure_optim_, n_live, obs.c_str());
    }
    for (const auto& kv : held) {
      const Frame& f = *kv.second;
      fprintf(out, "frame %d %zu\ntypes", f.id(), f.num_features_);
      for (size_t i = 0; i < f.num_features_; ++i) fprintf(out, " %d", (int)f.type_vec_[i]);
      fprintf(out, "\ntracks");
      for (size_t i = 0; i < f.num_features_; ++i) fprintf(out, " %d", f.track_id_vec_[i]);
      fprintf(out, "\nseedrefs");
      for (size_t i = 0; i < f.num_features_; ++i) {
        const Frame::SeedRef& r = f.seed_ref_vec_[i];
        fprintf(out, " %d %d", r.keyframe ? r.keyframe->id() : -1, r.seed_id);
      }
      fprintf(out, "\n");
    }
    fprintf(out, "alive");
    for (const auto& kv : frames) fprintf(out, " %d %d", kv.first, kv.second.expired() ? 0 : 1);
    fprintf(out, "\n");
  }
};

template <class T> void write_row(FILE* out, const char* name, const T* v, size_t n, const char* format)
{
  fprintf(out, "%s", name);
  for (size_t i = 0; i < n; ++i) { fputc(' ', out); fprintf(out, format, v[i]); }
  fputc('\n', out);
}
}  // namespace

int main(int argc, char** argv)
{
  if (argc < 3) { fprintf(stderr, "usage: %s <script.txt> <dump.txt> [--device]\n", argv[0]); return 2; }
  const bool device = argc > 3 && std::string(argv[3]) == "--device";
  std::ifstream in(argv[1]);
  if (!in) { fprintf(stderr, "landmarks_tool: cannot read %s\n", argv[1]); return 3; }
  Scene sc;
  sc.out = fopen(argv[2], "w");
  if (!sc.out) { fprintf(stderr, "landmarks_tool: cannot write %s\n", argv[2]); return 4; }
  svoh_ctx* ctx = nullptr;
  if (device && svoh_create(0, &ctx) != SVOH_OK) { fprintf(stderr, "svoh_create: %s\n", svoh_last_error_string(nullptr)); return 5; }
  int rc = 0;
  try {
    // finish() is host bookkeeping on the arrays it is handed and never touches the context; the constructor only refuses a null one
    // (compute() has no CPU fallback).  Without --device it gets a pointer that nothing dereferences.
    static char no_device;
    StereoTriangulationHip stereo(ctx ? ctx : reinterpret_cast<svoh_ctx*>(&no_device), StereoTriangulationOptions(), nullptr);
    int next_point_id = 1 << 20;   // as the harnesses count (the triangulation's points count from 0)
    std::string line;
    while (std::getline(in, line)) {
      std::istringstream ls(line);
      std::string ev;
      if (!(ls >> ev)) continue;
      auto geti = [&]() { long long v; if (!(ls >> v)) throw std::logic_error("script: integer expected in: " + line.substr(0, 60)); return v; };
      auto getd = [&]() { double v; if (!(ls >> v)) throw std::logic_error("script: number expected in: " + line.substr(0, 60)); return v; };
      std::string what_event = ev;
      try {
        if (ev == "frame") {
          const int id = (int)geti();
          const size_t n = (size_t)geti(), cap = (size_t)geti();
          if (n > cap) throw std::logic_error("script: frame larger than its capacity");
          auto f = std::make_shared<Frame>();
          f->id_ = id; f->num_features_ = n;
          f->T_f_w_.q.w = getd(); f->T_f_w_.q.x = getd(); f->T_f_w_.q.y = getd(); f->T_f_w_.q.z = getd();
          f->T_f_w_.t.x = getd(); f->T_f_w_.t.y = getd(); f->T_f_w_.t.z = getd();
          f->px_vec_.assign(2 * cap, 0.0); f->f_vec_.assign(3 * cap, 0.0); f->grad_vec_.assign(2 * cap, 0.0); f->level_vec_.assign(cap, 0);
          f->score_vec_.assign(cap, 0.0); f->type_vec_.assign(cap, SVOH_FT_OUTLIER); f->invmu_sigma2_a_b_vec_.assign(4 * cap, 0.0);
          f->landmark_vec_.assign(cap, nullptr); f->seed_ref_vec_.assign(cap, Frame::SeedRef()); f->track_id_vec_.assign(cap, -1);
          sc.held[id] = f; sc.frames[id] = f;
        } else if (ev == "grow") {
          const FramePtr f = sc.frame((int)geti());
          const size_t n = (size_t)geti();
          if (n < f->num_features_ || n > f->type_vec_.size()) throw std::logic_error("script: grow beyond the frame's capacity");
          f->num_features_ = n;
        } else if (ev == "feat") {
          const FramePtr f = sc.frame((int)geti());
          const size_t i = (size_t)geti();
          if (i >= f->type_vec_.size()) throw std::logic_error("script: feature beyond the frame's capacity");
          f->type_vec_[i] = (uint8_t)geti();
          for (int c = 0; c < 3; ++c) f->f_vec_[3 * i + c] = getd();
          f->invmu_sigma2_a_b_vec_[4 * i] = getd();
        } else if (ev == "seedref") {
          const FramePtr f = sc.frame((int)geti());
          const size_t i = (size_t)geti();
          const FramePtr kf = sc.frame((int)geti());
          const int sid = (int)geti();
          if (i >= f->seed_ref_vec_.size() || sid < 0 || (size_t)sid >= kf->num_features_) throw std::logic_error("script: seed reference out of range");
          f->seed_ref_vec_[i].keyframe = kf; f->seed_ref_vec_[i].seed_id = sid;
        } else if (ev == "track") {
          const FramePtr f = sc.frame((int)geti());
          const size_t i = (size_t)geti();
          f->track_id_vec_.at(i) = (int)geti();
        } else if (ev == "point") {
          auto p = std::make_shared<Point>();
          p->id_ = (int)geti();
          p->pos_.x = getd(); p->pos_.y = getd(); p->pos_.z = getd();
          p->last_structure_optim_ = (int)geti();
          sc.registered[p->id_] = p;
        } else if (ev == "landmark") {
          const FramePtr f = sc.frame((int)geti());
          const size_t i = (size_t)geti();
          const int pid = (int)geti();
          // the script's own point, or one a mirror made: then some live frame carries it
          PointPtr p = sc.registered.count(pid) ? sc.registered[pid] : nullptr;
          for (const auto& kv : sc.frames) {
            if (p) break;
            if (const FramePtr g = kv.second.lock())
              for (size_t k = 0; k < g->num_features_ && !p; ++k)
                if (g->landmark_vec_[k] && g->landmark_vec_[k]->id() == pid) p = g->landmark_vec_[k];
          }
          if (!p) throw std::logic_error("script: no point " + std::to_string(pid));
          f->landmark_vec_.at(i) = p;
        } else if (ev == "obs") {
          const int pid = (int)geti();
          what_event += " " + std::to_string(pid);
          const FramePtr f = sc.frame((int)geti());
          sc.registered.at(pid)->addObservation(f, (size_t)geti());
        } else if (ev == "upgrade") {
          const int fid = (int)geti();
          what_event += " " + std::to_string(fid);
          std::vector<size_t> edgelets;
          const size_t n = upgradeSeedsToFeatures(sc.frame(fid), &next_point_id, &edgelets);
          fprintf(sc.out, "upgraded %d %zu %zu", fid, n, edgelets.size());
          for (size_t e : edgelets) fprintf(sc.out, " %zu", e);
          fprintf(sc.out, "\n");
        } else if (ev == "stereo") {
          const FramePtr f0 = sc.frame((int)geti()), f1 = sc.frame((int)geti());
          StereoTriangulationHip::Job job;
          job.n_old = (size_t)geti(); job.n_new = (size_t)geti(); job.n_desired = (size_t)geti();
          const size_t n = job.n_new;
          if (f0->num_features_ != job.n_old + n) throw std::logic_error("script: the first frame does not end with the new features");
          if (f1->num_features_ + std::min(job.n_desired, n) > f1->type_vec_.size()) throw std::logic_error("script: no room in the second frame");
          std::vector<int32_t> result(n);
          std::vector<double> depth(n), px_cur(2 * n, 0.0), f_cur(3 * n), A(4 * n, 0.0);
          for (size_t k = 0; k < n; ++k) {
            const size_t i = (size_t)geti();
            if (i < job.n_old || i >= job.n_old + n) throw std::logic_error("script: index outside the new features");
            job.indices.push_back(i);
          }
          for (size_t k = 0; k < n; ++k) result[k] = (int32_t)geti();
          for (size_t k = 0; k < n; ++k) depth[k] = getd();
          for (size_t k = 0; k < 3 * n; ++k) f_cur[k] = getd();
          for (size_t k = 0; k < n; ++k) A[4 * k] = A[4 * k + 3] = 1.0;
          stereo.finish(f0, f1, job, result.data(), depth.data(), px_cur.data(), f_cur.data(), A.data());
          fprintf(sc.out, "stereo %zu %zu %zu\n", stereo.last_n_succeeded_, stereo.last_n_failed_, f1->num_features_);
        } else if (ev == "init") {
          const FramePtr cur = sc.frame((int)geti()), ref = sc.frame((int)geti());
          const double depth = getd();
          Transformation T;
          T.q.w = getd(); T.q.x = getd(); T.q.y = getd(); T.q.z = getd(); T.t.x = getd(); T.t.y = getd(); T.t.z = getd();
          const size_t m = (size_t)geti();
          initialization_utils::FeatureMatches matches;
          std::vector<double> pts;
          for (size_t k = 0; k < m; ++k) {
            const size_t ic = (size_t)geti(), ir = (size_t)geti();
            if (ic >= cur->num_features_ || ir >= ref->num_features_) throw std::logic_error("script: match out of range");
            matches.emplace_back(ic, ir);
            for (int c = 0; c < 3; ++c) pts.push_back(getd());
          }
          const double scale = initialization_utils::rescaleAndInitializePoints(cur, ref, matches, pts, T, depth);
          const Transformation& Tc = cur->T_f_w_;
          fprintf(sc.out, "init %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", scale, Tc.q.w, Tc.q.x, Tc.q.y, Tc.q.z, Tc.t.x, Tc.t.y, Tc.t.z);
        } else if (ev == "remove") {
          removeObservationsOf(*sc.frame((int)geti()));
        } else if (ev == "clearrefs") {
          for (Frame::SeedRef& r : sc.frame((int)geti())->seed_ref_vec_) r = Frame::SeedRef();
        } else if (ev == "drop") {
          sc.held.erase((int)geti());
        } else if (ev == "structure") {
          int max_n_pts = (int)geti();
          const size_t nf = (size_t)geti();
          auto bundle = std::make_shared<FrameBundle>();
          for (size_t k = 0; k < nf; ++k) bundle->frames_.push_back(sc.frame((int)geti()));
          const size_t n_scripted = (size_t)geti();
          std::map<std::pair<size_t, int>, svoh::Vec3> scripted;
          for (size_t k = 0; k < n_scripted; ++k) {
            const size_t place = (size_t)geti();
            const int pid = (int)geti();
            const double x = getd(), y = getd(), z = getd();
            scripted[std::make_pair(place, pid)] = svoh::Vec3{ x, y, z };
          }
          size_t n_total = 0;
          if (device) {
            n_total = optimizeStructure(ctx, bundle, max_n_pts, 5);
          } else if (max_n_pts != 0) {   // optimizeStructure's loop (svo_hip_host.cpp), gather's output in place of the launch
            StructureBatch b;
            for (size_t place = 0; place < nf; ++place) {
              const Frame& frame = *bundle->frames_[place];
              const int max_in = max_n_pts;
              max_n_pts = b.gather(frame, max_n_pts);
              fprintf(sc.out, "step %d %d %d %zu %zu %zu\n", frame.id(), max_in, max_n_pts, b.pts.size(), b.pts.empty() ? (size_t)0 : b.views.size(),
                      b.pts.empty() ? (size_t)0 : b.obs_view.size());
              if (b.pts.empty()) continue;
              fprintf(sc.out, "pts");
              for (const PointPtr& p : b.pts) fprintf(sc.out, " %d", p->id());
              fprintf(sc.out, "\nviews");
              for (const svoh_se3& v : b.views) { for (double q : v.q) fprintf(sc.out, " %.17g", q); for (double t : v.t) fprintf(sc.out, " %.17g", t); }
              fprintf(sc.out, "\n");
              write_row(sc.out, "obs_begin", b.obs_begin.data(), b.obs_begin.size(), "%d");
              write_row(sc.out, "obs_view", b.obs_view.data(), b.obs_view.size(), "%d");
              write_row(sc.out, "obs_f", b.obs_f.data(), b.obs_f.size(), "%.17g");
              write_row(sc.out, "pos", b.pos.data(), b.pos.size(), "%.17g");
              std::vector<double> pos_out(b.pos);
              for (size_t k = 0; k < b.pts.size(); ++k) {
                auto it = scripted.find(std::make_pair(place, b.pts[k]->id()));
                if (it != scripted.end()) { pos_out[3 * k] = it->second.x; pos_out[3 * k + 1] = it->second.y; pos_out[3 * k + 2] = it->second.z; }
              }
              b.apply(pos_out.data());
              n_total += b.pts.size();
            }
          }
          fprintf(sc.out, "structure %zu\n", n_total);
        } else if (ev == "state") {
          sc.state();
        } else {
          throw std::logic_error("script: unknown event " + ev);
        }
      } catch (const std::logic_error&) {
        throw;   // a broken script or a misuse of the standard library: not a mirror's refusal
      } catch (const std::runtime_error& e) {
        fprintf(stderr, "landmarks_tool: %s: %s\n", what_event.c_str(), e.what());
        fprintf(sc.out, "throw %s\n", what_event.c_str());
        break;
      }
    }
    sc.state();
  } catch (const std::exception& e) {
    fprintf(stderr, "landmarks_tool: %s\n", e.what());
    rc = 1;
  }
  fclose(sc.out);
  sc.held.clear(); sc.registered.clear();
  if (ctx) svoh_destroy(ctx);
  return rc;
}
