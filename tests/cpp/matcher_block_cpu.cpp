// The matcher's staging blocks (csrc/svoh_matcher_block.h) printed column by column: every layout the entries of matcher.hip
// build, at the unit counts where 4-byte and 1-byte columns cross a 64-byte boundary.  tests/test_matcher_block_cpu.py compares
// the output with tests/matcher_block_layout.py.  Stand-alone: the header and nothing else of the library.
//   case <layout> key=value ...
//   col <name> <offset>            (in block order)
//   marks <in_total> <back_from> <end> <total>
#include <cstdio>

#include "../../svo_pro_universal_amd/csrc/svoh_matcher_block.h"

using namespace svoh;

static const char* const kName[kSlotCount] = {
  "views", "T_cur_ref", "chain_begin", "chain_idx", "ref_frame_idx", "cur_frame_idx", "feature_index", "px", "f", "grad", "level", "type",
  "depth", "px_cur", "landmark_xyz", "d_inv", "state", "result", "f_cur", "search_level", "h_inv", "A_cur_ref", "success", "depth_out",
  "n_success", "steps_succeeded", "step_result", "step_success",
};

// svoh_feature_batch by its members, as the layouts name it
struct Batch {
  const int32_t* ref_frame_idx; const double* px; const double* f; const double* grad; const int32_t* level; uint8_t* type;
  const int32_t* cur_frame_idx;
};

static void print(const MatcherBlock& b)
{
  for (int k = 0; k < b.n_cols; ++k) std::printf("col %s %zu\n", kName[b.order[k]], b.off((MatcherSlot)b.order[k]));
  std::printf("marks %zu %zu %zu %zu\n", b.in_total, b.back_from, b.end, b.total);
}

int main()
{
  // the layouts read which optional arrays are given, never the arrays: any non-NULL pointer stands for "given"
  static double some_double;
  static int32_t some_int;
  static uint8_t some_byte;
  const int ns[] = { 1, 15, 16, 17, 63, 64, 65 };
  const int view_counts[] = { 2, 5 };
  const size_t view_sizes[] = { 432, 472 };   // sizeof(DevFrameView), sizeof(DevFrameViewWide)
  const size_t rigid_bytes = 56;              // sizeof(Rigid)
  for (int n : ns) for (int nv : view_counts) for (size_t vb : view_sizes) {
    for (int cur = 0; cur < 2; ++cur) {
      Batch fb = { &some_int, &some_double, &some_double, &some_double, &some_int, &some_byte, cur ? &some_int : nullptr };
      for (int opt = 0; opt < 2; ++opt) {
        {
          MatcherArrays c;
          c.depth = &some_double; c.px_cur = &some_double; c.result = &some_int; c.landmark_xyz = opt ? &some_double : nullptr;
          MatcherBlock b;
          layout_matcher_batch(b, false, (size_t)n, &some_byte, vb * nv, fb, c, false);
          std::printf("case direct n=%d views=%d view_bytes=%zu cur_idx=%d landmark_xyz=%d\n", n, nv, vb, cur, opt);
          print(b);
        }
        {
          MatcherArrays c;
          c.state = &some_double; c.success = &some_byte; c.px_cur = opt ? &some_double : nullptr;
          MatcherBlock b;
          layout_matcher_batch(b, true, (size_t)n, &some_byte, vb * nv, fb, c, false);
          std::printf("case seeds n=%d views=%d view_bytes=%zu cur_idx=%d px_cur=%d\n", n, nv, vb, cur, opt);
          print(b);
        }
        for (int with_T = 0; with_T < 2; ++with_T) {
          MatcherArrays c;
          c.result = &some_int; c.depth_out = &some_double; c.d_inv = opt ? &some_double : nullptr;
          const size_t t_bytes = with_T ? rigid_bytes * (size_t)(nv - 1) : 0;   // one reference frame, nv - 1 current frames
          MatcherBlock b;
          layout_epipolar_batch(b, (size_t)n, &some_byte, vb * nv, with_T ? &some_byte : nullptr, t_bytes, fb, c, false);
          std::printf("case epipolar n=%d views=%d view_bytes=%zu cur_idx=%d d_inv=%d t_bytes=%zu\n", n, nv, vb, cur, opt, t_bytes);
          print(b);
        }
      }
    }
    // the chain: 3 reference frames (the table holds 3 + nv views), 0 and 4 links, step outputs over 0 and 2 steps
    const int links[] = { 0, 4 }, steps[] = { 0, 2 };
    Batch fb = { &some_int, &some_double, &some_double, &some_double, &some_int, &some_byte, nullptr };
    for (int nl : links) for (int ms : steps) for (int sr = 0; sr < 2; ++sr) for (int ss = 0; ss < 2; ++ss) {
      const size_t n_steps_out = (sr || ss) ? (size_t)n * ms : 0;
      MatcherBlock b;
      layout_seed_chain(b, (size_t)n, &some_byte, vb * (3 + nv), 3, &some_int, (size_t)nl, &some_int, fb, &some_double, &some_int,
                        sr ? &some_int : nullptr, ss ? &some_byte : nullptr, n_steps_out);
      std::printf("case chain n=%d views=%d view_bytes=%zu n_ref=3 links=%d max_steps=%d step_result=%d step_success=%d\n", n, 3 + nv, vb, nl, ms, sr, ss);
      print(b);
    }
    for (int seeds = 0; seeds < 2; ++seeds) for (int outputs = 0; outputs < 2; ++outputs) for (int resident = 0; resident < 2; ++resident) {
      MatcherBlock b;
      layout_matcher_stage(b, seeds != 0, (size_t)n, (size_t)nv, vb, outputs != 0, resident != 0);
      std::printf("case staged n=%d views=%d view_bytes=%zu seeds=%d outputs=%d resident=%d\n", n, nv, vb, seeds, outputs, resident);
      print(b);
      // what svoh_matcher_stage hands out: the pinned block's columns but the device-only ones
      uint8_t* const h = &some_byte;
      for (int k = 0; k < b.n_cols; ++k) {
        const MatcherSlot s = (MatcherSlot)b.order[k];
        const void* p = b.staged(h, s);
        if (p) std::printf("handed %s %zu\n", kName[s], (size_t)(static_cast<const uint8_t*>(p) - h));
      }
    }
  }
  return 0;
}
