// svoh_matcher_block.h -- the staging block of a matcher batch, described once (matcher.hip's host side).
// Host only: plain C++17 without a HIP type, so that tests/cpp/matcher_block_cpu.cpp compiles it with g++.
//
// Every matcher entry sends a batch through ONE 64-byte-aligned block [views | inputs | in/out | outputs | count] that exists
// twice, in a pinned buffer and in a device buffer.  A block is an ordered list of columns; a column has a slot (which kernel
// argument or svoh_matcher_stage_t member it feeds), a byte count, a direction and, for a batch of caller arrays, the caller's
// pointer.  From that list come the gather into the pinned block, the kernel arguments, the scatter to the caller's arrays (at
// once or at svoh_matcher_collect) and the pointers svoh_matcher_stage hands out.  The layout_* functions below are the layouts
// there are; tests/matcher_block_layout.py restates them column by column.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace svoh {

// the geometry of a matcher launch (the kernels' template parameter G8 takes these values): one lane per unit, eight lanes per
// unit, the packed kernels (large batches, kPkThreads units per block), one wave per unit (the epipolar scan 64 steps at a time)
enum MatcherGeometry : int { kGeomOneLane = 0, kGeomEightLanes = 1, kGeomPacked = 2, kGeomOneWave = 3 };
// units per 64-thread block of the per-unit geometries
inline int units_per_block(MatcherGeometry g) { return g == kGeomEightLanes ? 8 : (g == kGeomOneWave ? 1 : 64); }

enum MatcherSlot : uint8_t {
  kSlotViews, kSlotTCurRef, kSlotChainBegin, kSlotChainIdx,                                            // tables
  kSlotRefIdx, kSlotCurIdx, kSlotFeatIdx, kSlotPx, kSlotF, kSlotGrad, kSlotLevel, kSlotType,           // svoh_feature_batch
  kSlotDepth, kSlotPxCur, kSlotLandmark, kSlotDInv, kSlotState,                                        // per-unit arguments
  kSlotResult, kSlotFCur, kSlotSearchLevel, kSlotHInv, kSlotA, kSlotSuccess, kSlotDepthOut,            // outputs
  kSlotNSuccess, kSlotStepsOk, kSlotStepResult, kSlotStepSuccess,
  kSlotCount
};

enum ColumnDir : uint8_t {
  kColIn,      // gathered from the caller's array
  kColInOut,   // gathered from it, and scattered to it once the block is back
  kColOut,     // scattered to it, where the caller gave one
  kColDevice,  // exists in the device block only: nothing is handed out, gathered or scattered
  kColCaller,  // a device batch's: the kernel reads and writes the caller's array in place, the block has no room for it
};

// the caller's per-unit arrays of a batch besides the svoh_feature_batch's own, by name; NULL = not given
struct MatcherArrays {
  const double* depth = nullptr; const double* landmark_xyz = nullptr;   // direct: in (landmark_xyz: the pixelwise warp)
  const double* d_inv = nullptr; double* depth_out = nullptr;            // epipolar: in, out
  double* px_cur = nullptr;                                              // direct: in / out; seeds, epipolar: out
  double* state = nullptr; uint8_t* success = nullptr;                   // seeds: in / out, out
  int32_t* result = nullptr; double* f_cur = nullptr; int32_t* search_level = nullptr; double* h_inv = nullptr; double* A_cur_ref = nullptr;
  int32_t* n_success = nullptr;                                          // seeds: one number for the batch
};

struct MatcherBlock {
  struct Column { size_t off = 0, bytes = 0; void* host = nullptr; ColumnDir dir = kColIn; bool present = false; };   // host: the caller's array, or NULL
  Column col[kSlotCount];      // by slot; a slot stands at most once in a block
  uint8_t order[kSlotCount];   // the slots in the order they were added
  int n_cols = 0;
  size_t total = 0;            // bytes of the block
  size_t in_total = 0;         // the end of what is uploaded
  size_t back_from = 0;        // the first byte that comes back ...
  size_t end = 0;              // ... and the end of what does

  // appends a column and returns its offset; the running total is rounded up to 64 (kColCaller: no room, `host` may be NULL)
  size_t add(MatcherSlot s, size_t bytes, ColumnDir dir, const void* host = nullptr)
  {
    if (dir == kColCaller) bytes = 0;
    col[s] = Column{ total, bytes, const_cast<void*>(host), dir, true };
    order[n_cols++] = s;
    if (dir != kColCaller) total = (total + bytes + 63) & ~(size_t)63;
    return col[s].off;
  }
  bool has(MatcherSlot s) const { return col[s].present; }
  size_t off(MatcherSlot s) const { return col[s].off; }
  // where the kernels find slot s with the block at `d`: in the block, at the caller's own pointer (device batch), or NULL
  void* at(uint8_t* d, MatcherSlot s) const { return !col[s].present ? nullptr : (col[s].dir == kColCaller ? col[s].host : static_cast<void*>(d + col[s].off)); }
  // what svoh_matcher_stage hands out for slot s with the pinned block at `h` (and what the batch must then name): NULL for a
  // column the block does not have or has on the device only
  void* staged(uint8_t* h, MatcherSlot s) const { return (col[s].present && col[s].dir <= kColOut) ? static_cast<void*>(h + col[s].off) : nullptr; }
  // the caller's input arrays into the pinned block
  void gather(uint8_t* h) const
  {
    for (int k = 0; k < n_cols; ++k) {
      const Column& c = col[order[k]];
      if (c.dir <= kColInOut && c.host) memcpy(h + c.off, c.host, c.bytes);
    }
  }
  // copy(dst, src, bytes) for every column that goes back to an array the caller gave: called once the block is back in `h`,
  // or to remember the copies until then (a deferred batch)
  template <class Copy>
  void scatter(const uint8_t* h, Copy&& copy) const
  {
    for (int k = 0; k < n_cols; ++k) {
      const Column& c = col[order[k]];
      if ((c.dir == kColInOut || c.dir == kColOut) && c.host && c.bytes) copy(c.host, h + c.off, c.bytes);
    }
  }
};

// ---- the layouts ---------------------------------------------------------------------------------------------------------
// `Batch` is svoh_feature_batch (include/svo_hip.h), named by its members only.  on_device: the batch's arrays are device
// arrays, read and written in place (kColCaller); the block then holds the tables and the success count only.

// A batch of caller arrays: add(slot, bytes per unit, direction, array) for the columns; the views, the (optional) T_cur_ref table
// and the svoh_feature_batch's own columns are the same in every such block
template <class Batch>
struct BatchColumns {
  MatcherBlock& b; size_t n; bool on_device;
  void add(MatcherSlot s, size_t per_unit, ColumnDir dir, const void* p) const { b.add(s, per_unit * n, on_device ? kColCaller : dir, p); }
  void optional(MatcherSlot s, size_t per_unit, ColumnDir dir, const void* p) const { if (on_device || p) add(s, per_unit, dir, p); }
  void head(const void* views, size_t views_bytes, const void* T_cur_ref, size_t T_bytes, const Batch& fb, ColumnDir type_dir) const
  {
    b.add(kSlotViews, views_bytes, kColIn, views);
    if (T_cur_ref) b.add(kSlotTCurRef, T_bytes, kColIn, T_cur_ref);
    add(kSlotRefIdx, 4, kColIn, fb.ref_frame_idx); optional(kSlotCurIdx, 4, kColIn, fb.cur_frame_idx);
    add(kSlotPx, 16, kColIn, fb.px); add(kSlotF, 24, kColIn, fb.f); add(kSlotGrad, 16, kColIn, fb.grad); add(kSlotLevel, 4, kColIn, fb.level);
    add(kSlotType, 1, type_dir, fb.type);
  }
};

// svoh_match_direct_batch[_pixelwise] / svoh_update_seeds_batch[_ex] over caller arrays:
// [views | ref idx | (cur idx) | px | f | grad | level | type | seeds: state; direct: depth, px_cur | (landmark_xyz) ||
//  result | f_cur | search_level | h_inv | A_cur_ref | success | (seeds: px_cur) | n_success]; from `type` up to n_success comes back
// (a direct batch's type with the rest: it stays in the block)
template <class Batch>
inline void layout_matcher_batch(MatcherBlock& b, bool seeds, size_t n, const void* views, size_t views_bytes, const Batch& fb,
                                 const MatcherArrays& c, bool on_device)
{
  const BatchColumns<Batch> col{ b, n, on_device };
  col.head(views, views_bytes, nullptr, 0, fb, seeds ? kColInOut : kColIn);
  b.back_from = b.off(kSlotType);
  if (seeds) col.add(kSlotState, 32, kColInOut, c.state);
  else { col.add(kSlotDepth, 8, kColIn, c.depth); col.add(kSlotPxCur, 16, kColInOut, c.px_cur); }
  col.optional(kSlotLandmark, 24, kColIn, c.landmark_xyz);
  b.in_total = b.total;
  col.add(kSlotResult, 4, kColOut, c.result); col.add(kSlotFCur, 24, kColOut, c.f_cur); col.add(kSlotSearchLevel, 4, kColOut, c.search_level);
  col.add(kSlotHInv, 8, kColOut, c.h_inv); col.add(kSlotA, 32, kColOut, c.A_cur_ref); col.add(kSlotSuccess, 1, kColOut, c.success);
  if (seeds) col.optional(kSlotPxCur, 16, kColOut, c.px_cur);   // matcher px_cur_ of the seed update (output only)
  b.end = b.add(kSlotNSuccess, sizeof(int32_t), kColOut);
}

// svoh_epipolar_match_batch: [views | (T_cur_ref) | ref idx | (cur idx) | px | f | grad | level | type | (d_inv) ||
//  result | depth | px_cur | f_cur | search_level | h_inv | A_cur_ref]; the outputs come back
template <class Batch>
inline void layout_epipolar_batch(MatcherBlock& b, size_t n, const void* views, size_t views_bytes, const void* T_cur_ref,
                                  size_t T_bytes, const Batch& fb, const MatcherArrays& c, bool on_device)
{
  const BatchColumns<Batch> col{ b, n, on_device };
  col.head(views, views_bytes, T_cur_ref, T_bytes, fb, kColIn);
  col.optional(kSlotDInv, 24, kColIn, c.d_inv);
  b.in_total = b.total;
  col.add(kSlotResult, 4, kColOut, c.result); col.add(kSlotDepthOut, 8, kColOut, c.depth_out); col.add(kSlotPxCur, 16, kColOut, c.px_cur);
  col.add(kSlotFCur, 24, kColOut, c.f_cur); col.add(kSlotSearchLevel, 4, kColOut, c.search_level); col.add(kSlotHInv, 8, kColOut, c.h_inv);
  col.add(kSlotA, 32, kColOut, c.A_cur_ref);
  b.back_from = b.off(kSlotResult);
  b.end = b.total;
}

// svoh_update_seeds_chain (host arrays only): [views (reference, then chain frames) | chain_begin | chain_idx | ref idx | px | f |
//  grad | level | type | state || steps_succeeded | (step_result) | (step_success)]; from `type` on comes back
template <class Batch>
inline void layout_seed_chain(MatcherBlock& b, size_t n, const void* views, size_t views_bytes, size_t n_ref_frames,
                              const int32_t* chain_begin, size_t n_links, const int32_t* chain_idx, const Batch& fb, double* state,
                              int32_t* steps_succeeded, int32_t* step_result, uint8_t* step_success, size_t n_steps_out)
{
  b.add(kSlotViews, views_bytes, kColIn, views);
  b.add(kSlotChainBegin, 4 * (n_ref_frames + 1), kColIn, chain_begin); b.add(kSlotChainIdx, 4 * n_links, kColIn, chain_idx);
  b.add(kSlotRefIdx, 4 * n, kColIn, fb.ref_frame_idx);
  b.add(kSlotPx, 16 * n, kColIn, fb.px); b.add(kSlotF, 24 * n, kColIn, fb.f); b.add(kSlotGrad, 16 * n, kColIn, fb.grad); b.add(kSlotLevel, 4 * n, kColIn, fb.level);
  b.back_from = b.add(kSlotType, n, kColInOut, fb.type);
  b.add(kSlotState, 32 * n, kColInOut, state);
  b.in_total = b.total;
  b.add(kSlotStepsOk, 4 * n, kColOut, steps_succeeded);
  if (step_result) b.add(kSlotStepResult, 4 * n_steps_out, kColOut, step_result);
  if (step_success) b.add(kSlotStepSuccess, n_steps_out, kColOut, step_success);
  b.end = b.total;
}

// svoh_matcher_stage: the caller writes the inputs into the pinned block and reads the outputs from it, so no column has a
// caller array.  [views (max) | ref idx | cur idx | resident: feature_index; else: px, f, grad, level | (direct: depth) | type |
//  direct: px_cur; seeds: state || result | success | (match outputs: (seeds: px_cur), f_cur, search_level, h_inv, A_cur_ref) |
//  n_success | resident: px, f, grad, level on the device only, behind everything that crosses PCIe]; from `type` up to n_success
// comes back.  A direct batch always has the match outputs.
inline void layout_matcher_stage(MatcherBlock& b, bool seeds, size_t n, size_t max_views, size_t view_bytes, bool want_outputs,
                                 bool resident)
{
  const auto columns = [&](ColumnDir dir) { b.add(kSlotPx, 16 * n, dir); b.add(kSlotF, 24 * n, dir); b.add(kSlotGrad, 16 * n, dir); b.add(kSlotLevel, 4 * n, dir); };
  b.add(kSlotViews, view_bytes * max_views, kColIn);
  b.add(kSlotRefIdx, 4 * n, kColIn); b.add(kSlotCurIdx, 4 * n, kColIn);
  if (resident) b.add(kSlotFeatIdx, 4 * n, kColIn);
  else columns(kColIn);
  if (!seeds) b.add(kSlotDepth, 8 * n, kColIn);
  b.back_from = b.add(kSlotType, n, kColInOut);
  if (seeds) b.add(kSlotState, 32 * n, kColInOut);
  else b.add(kSlotPxCur, 16 * n, kColInOut);
  b.in_total = b.total;
  b.add(kSlotResult, 4 * n, kColOut); b.add(kSlotSuccess, n, kColOut);
  if (want_outputs || !seeds) {
    if (seeds) b.add(kSlotPxCur, 16 * n, kColOut);
    b.add(kSlotFCur, 24 * n, kColOut); b.add(kSlotSearchLevel, 4 * n, kColOut); b.add(kSlotHInv, 8 * n, kColOut); b.add(kSlotA, 32 * n, kColOut);
  }
  b.end = b.add(kSlotNSuccess, sizeof(int32_t), kColOut);
  if (resident) columns(kColDevice);
}

}  // namespace svoh
