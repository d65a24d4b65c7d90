// svoh_align_block.h -- the staged block of an alignment launch, its feature workspace and its place in the launch queue, each
// described once (sparse_align.hip's host side).  Host only: plain C++17 without a HIP type, so that tests/cpp/align_block_cpu.cpp
// compiles it with g++.  tests/align_block_layout.py restates the layouts; tests/test_align_queue_cpu.py replays launch sequences.
#pragma once
#include <cstddef>
#include <cstdint>

namespace svoh {

// ---- the staged block --------------------------------------------------------------------------------------------------------
// [n_desc problem descriptors | n_cams_total camera descriptors | (256-aligned) 512 bytes of control: the work-queue head, and at
//  +256 one arrival counter per clustered problem | per uploaded camera: px 16n, f 24n, pos_world 24n, flags n, rounded up to 64,
//  and behind a camera with pos_seed_unit its units, 4n rounded up to 64 | the job table of those cameras, rounded up to 64]
// The block exists twice per slot, pinned and on the device; one upload of [0, used) carries it.  The control words are zeroed
// on the host.  `reserve` is what pass 1 of a launch asks of both buffers (a camera with units counts 64 bytes for its entry of
// the job table, more than the entry takes), `used` what pass 2 has placed.
constexpr size_t kAlignCtlBytes = 512;       // the control words ...
constexpr size_t kAlignBarOff = 256;         // ... and where the cluster arrival counters lie in them
inline size_t align_round64(size_t b) { return (b + 63) & ~(size_t)63; }

// a camera's four columns in its uploaded piece (n features), and the piece's length
struct AlignCamColumns {
  size_t px, f, pos, flags, stride;
  explicit AlignCamColumns(size_t n) : px(0), f(n * 16), pos(n * 40), flags(n * 64), stride(align_round64(n * 65)) {}
};
inline size_t align_units_stride(size_t n) { return align_round64(n * 4); }

// share s of S of a camera's n features: [lo, hi)
struct AlignShare {
  size_t lo, hi;
  AlignShare(int64_t n, int s, int S) : lo((size_t)(n * s / S)), hi((size_t)(n * (s + 1) / S)) {}
  size_t n() const { return hi - lo; }
};

struct AlignBlock {
  size_t cams_off = 0;     // the camera descriptors, behind the problem descriptors
  size_t ctl_off = 0;      // the control words: the queue head at ctl_off ...
  size_t bar_off = 0;      // ... the arrival counters of cluster mode
  size_t up_base = 0;      // the first uploaded camera
  size_t reserve = 0;      // bytes both buffers must hold
  size_t used = 0;         // the end of what has been placed: the upload's length
  // pass 1: room for a camera whose arrays go up, and for the units (and the job) of one with pos_seed_unit ...
  void size_camera(size_t n) { reserve += AlignCamColumns(n).stride; }
  void size_seed_units(size_t n) { reserve += align_units_stride(n) + 64; }
  // ... then, the cameras counted, the descriptors in front of them (problem_bytes / cam_bytes: sizeof(DevProblemDesc) / sizeof(DevCamDesc))
  void lay_out(size_t n_desc, size_t n_cams_total, size_t problem_bytes, size_t cam_bytes)
  {
    cams_off = problem_bytes * n_desc;
    ctl_off = (cams_off + cam_bytes * n_cams_total + 255) & ~(size_t)255;
    bar_off = ctl_off + kAlignBarOff;
    up_base = ctl_off + kAlignCtlBytes;
    reserve += up_base;
    used = up_base;
  }
  // pass 2: where the next piece lies
  size_t place_camera(size_t n) { const size_t at = used; used += AlignCamColumns(n).stride; return at; }
  size_t place_seed_units(size_t n) { const size_t at = used; used += align_units_stride(n); return at; }
  size_t place_job_table(size_t n_jobs, size_t job_bytes) { const size_t at = used; used += align_round64(job_bytes * n_jobs); return at; }
};

// ---- the feature workspace -----------------------------------------------------------------------------------------------------
// [wpk: kAlignWsPairs pairs of doubles per slot, pair-major | wsel: a byte per slot | wvis: a byte per slot | 256 bytes]
constexpr int kAlignWsPairs = 3;
struct AlignWorkspace {
  size_t slots, wpk_off, wsel_off, wvis_off, bytes;
  explicit AlignWorkspace(size_t n_features)
    : slots(n_features ? n_features : 1), wpk_off(0), wsel_off(slots * (size_t)kAlignWsPairs * 16), wvis_off(wsel_off + slots),
      bytes(slots * ((size_t)kAlignWsPairs * 16 + 2) + 256) {}
};

// ---- the launch queue ----------------------------------------------------------------------------------------------------------
// What the queue remembers between launches (svoh_internal.h, AlignQueue, says what each mechanism is for), without the HIP
// objects: an event is named by what it is.  place_block / place_launch say what the next launch gets, commit_launch what the
// queue remembers once its upload has been queued (the note_* functions: what it remembers of the events around that); the launch code
// carries the plan out and decides nothing.

// what the host waits for before it writes the pinned block of the launch before the last one again
enum AlignStagedWait : uint8_t { kAlignWaitNone, kAlignWaitStaged, kAlignWaitKernel0, kAlignWaitKernel1 };

struct AlignQueueState {
  unsigned launches_since_drain = 0;    // alignment launches queued since the host last waited for every stream of the queue
  unsigned desc_slot = 0;               // the descriptor blocks (pinned and device) of the most recent launch
  AlignStagedWait staged_wait = kAlignWaitNone;   // what the most recent launch recorded behind the upload of the launch before it
  bool block_read[2] = { false, false };   // an event lies behind the last kernel that read the device block of this slot (since the last drain)
  bool last_was_side = false;           // the most recent launch uploaded on the copy stream
  bool lane1_pending = false;           // a launch on lane 1 that the context's stream has not waited for (and no host wait has covered)
  bool lane1_wants_front = false;       // the front event was recorded and lane 1 has not waited for it yet
  bool chain = false;                   // the most recent work on either lane is a launch of the batch geometry that may be overlapped
  int last_lane = 0;                    // the lane of the most recent alignment launch
  unsigned long long lane1_launches = 0;
  unsigned long long side_launches = 0; // launches that took the side path (read by the test-hook library only)
};

// the host has waited for both lanes and for the copy stream
inline AlignQueueState align_drained(AlignQueueState s)
{
  s.lane1_pending = false;
  s.chain = false;
  s.last_lane = 0;
  s.launches_since_drain = 0;
  s.block_read[0] = s.block_read[1] = false;
  return s;
}

// The pinned blocks are reused in turn: the next launch takes the slot the last one did not take.  From the third launch of a
// queue on that block was last read by an upload nobody has waited for: the host waits for the event behind it, or drains.
enum AlignBlockWait : uint8_t { kAlignBlockFree, kAlignBlockWaitEvent, kAlignBlockDrain };
struct AlignBlockPlace { unsigned slot; AlignBlockWait wait; };
inline AlignBlockPlace place_block(const AlignQueueState& s)
{
  AlignBlockPlace p;
  p.slot = s.desc_slot ^ 1u;
  p.wait = s.launches_since_drain < 2 ? kAlignBlockFree : (s.staged_wait != kAlignWaitNone ? kAlignBlockWaitEvent : kAlignBlockDrain);
  return p;
}

// A device block, a result queue or a workspace that launches in flight may still use is replaced, and a stream of the queue is
// made, only once the host has waited for everything queued: whether that wait (a drain) is needed
inline bool align_busy(const AlignQueueState& s) { return s.launches_since_drain >= 1; }

// The two knobs (knob_set: the environment or the caller gave one).  SVOH_ALIGN_SIDE_COPIES: unset = launches whose upload is
// larger than the copy kernels' window (1 MB), 1 = every launch of the batch kind, 0 = none.  SVOH_ALIGN_OVERLAP: 0 = one lane.
constexpr size_t kAlignSideMinBytes = (size_t)1 << 20;
inline bool align_side_wanted(bool knob_set, int knob, size_t upload_bytes) { return knob_set ? knob != 0 : upload_bytes > kAlignSideMinBytes; }
inline bool align_overlap_wanted(bool knob_set, int knob) { return !knob_set || knob != 0; }

struct AlignLaunchPlan {
  unsigned slot = 0;             // descriptor blocks
  int lane = 0;                  // its lane
  bool overlapped = false;       // runs beside the launch before it
  bool side = false;             // uploads on the copy stream
  bool drain_first = false;      // the workspace of `grow_lane` is too small while the other lane may be busy: drain, grow it; the
  int grow_lane = 0;             //   rest of the plan is that of the first launch of a new queue
  // in front of the upload
  bool wait_front = false;       // lane 1 waits for the front event
  bool join = false;             // the context's stream waits for lane 1 (the first launch of a queue) ...
  bool record_front = false;     // ... and records the front event: the launch behind this one may take lane 1
  // the upload on the copy stream
  bool record_prev_kernel = false;      // the kernel event of the other slot, on the previous launch's lane: that launch recorded none
  bool wait_block_read = false;         // the copy stream waits for the kernel event of this slot
  bool record_staged_on_copy = false;   // the staged event behind the upload (the previous launch uploaded there too); else the host's next wait is for the other slot's kernel event
  // the upload on the launch's own lane
  bool record_staged_behind_prev = false;     // the staged event on the previous launch's lane, in front of the upload
  bool record_staged_behind_upload = false;   // the staged event on this lane, behind the upload
  // behind the kernel
  bool record_kernel = false;    // the kernel event of this slot; the download is held back
  bool record_lane1 = false;     // the lane-1 event
};

// lane_kind / side_kind: the launch is of the kind that may take the other lane / the copy stream (sparse_align.hip says which).
// ws_small[l]: lane l's workspace exists and is smaller than this launch needs.  lane1_has_launched: lane 1 exists and has run a launch.
inline AlignLaunchPlan place_launch(AlignQueueState s, bool lane_kind, bool side_kind, const bool ws_small[2], bool lane1_has_launched)
{
  AlignLaunchPlan p;
  p.slot = s.desc_slot ^ 1u;
  p.grow_lane = (lane_kind && s.chain && s.launches_since_drain >= 1 && s.last_lane == 0) ? 1 : 0;
  if (ws_small[p.grow_lane] && align_busy(s) && lane1_has_launched) {
    p.drain_first = true;
    s = align_drained(s);
  }
  p.overlapped = lane_kind && s.chain && s.launches_since_drain >= 1;
  p.lane = p.overlapped ? (s.last_lane ^ 1) : 0;
  p.wait_front = p.lane != 0 && s.lane1_wants_front;
  p.join = p.lane == 0 && !p.overlapped;
  p.record_front = p.join && lane_kind;
  p.side = side_kind && s.launches_since_drain >= 1;
  if (p.side) {
    p.record_prev_kernel = !s.block_read[p.slot ^ 1u];
    p.wait_block_read = s.block_read[p.slot];
    p.record_staged_on_copy = s.last_was_side;
  } else {
    p.record_staged_behind_prev = p.overlapped;
    p.record_staged_behind_upload = s.launches_since_drain >= 1 && !p.overlapped;
  }
  p.record_kernel = p.side;
  p.record_lane1 = p.lane != 0;
  return p;
}

// The queue's state follows the HIP calls one by one, so that a call that fails half way leaves what the calls before it made true:
// after the waits and records in front of the upload ...
inline void note_front_waited(AlignQueueState& s) { s.lane1_wants_front = false; }
inline void note_front_recorded(AlignQueueState& s) { s.lane1_wants_front = true; }
// ... once the launch's upload has been queued: the slot is taken (s: the state the plan was carried out on -- joined, drained, if the plan said so)
inline AlignQueueState commit_launch(AlignQueueState s, const AlignLaunchPlan& p, bool lane_kind)
{
  if (p.wait_front) s.lane1_wants_front = false;
  if (p.record_front) s.lane1_wants_front = true;
  if (p.side) {
    s.block_read[p.slot ^ 1u] = true;
    s.staged_wait = p.record_staged_on_copy ? kAlignWaitStaged : ((p.slot ^ 1u) ? kAlignWaitKernel1 : kAlignWaitKernel0);
    ++s.side_launches;
  } else {
    s.staged_wait = s.launches_since_drain >= 1 ? kAlignWaitStaged : kAlignWaitNone;
    s.block_read[p.slot] = false;  // (an event of an earlier kernel on this block says nothing about this one)
  }
  s.desc_slot = p.slot;
  s.last_was_side = p.side;
  ++s.launches_since_drain;
  s.last_lane = p.lane;
  s.chain = lane_kind;             // (a launch of another kind on the context's stream ends the queue like any other work there)
  if (p.lane) ++s.lane1_launches;
  return s;
}
// ... and behind the kernel, once the events of the plan have been recorded there
inline void note_kernel_recorded(AlignQueueState& s, const AlignLaunchPlan& p) { s.block_read[p.slot] = true; }
inline void note_lane1_recorded(AlignQueueState& s) { s.lane1_pending = true; }

}  // namespace svoh
