// The alignment's staged block, its feature workspace and its launch queue (csrc/svoh_align_block.h), stand-alone: the header and
// nothing else of the library.
//
//   align_block_cpu                 prints every offset of the block for the cases of tests/test_align_block_cpu.py, which compares
//                                   them with tests/align_block_layout.py:
//     case block problems=P cams=C n=N shares=S units=U
//     desc <cams_off> <ctl_off> <bar_off> <up_base>
//     cam <c> <at> <f> <pos> <flags> <stride>          (columns relative to the block)
//     units <c> <at>
//     jobs <at>
//     share <c> <s> <n> <px> <f> <pos> <flags>          (what the descriptor of share s points at, relative to the block)
//     total <reserve> <used>
//     case workspace feat=N
//     ws <slots> <wpk> <wsel> <wvis> <bytes>
//
//   align_block_cpu queue <overlap> <side> op ...      replays a sequence of calls through place_block / place_launch /
//                                   commit_launch as enqueue_align carries them out (tests/test_align_queue_cpu.py).  <overlap>,
//                                   <side>: the two knobs, 0, 1 or u (unset).  Operations:
//     b<ws>[:<upload bytes>][!]   a launch of the batch kind that needs <ws> bytes of workspace; !: one of its blocks must grow
//     s                           a launch of another kind (small, cluster, keyed)
//     e                           an evaluation: such a launch, and the host waits for it
//     x                           a call that fails in its fill pass, before its upload
//     j                           other work on the context's stream (join)
//     f                           a fetch (drain)
//                                 prints, per launch:  launch slot= lane= overlapped= side= wait=free|event|drain drained=
//                                 per failed call:     failed slot= wait=
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../svo_pro_universal_amd/csrc/svoh_align_block.h"

using namespace svoh;

// sizeof(DevProblemDesc), sizeof(DevCamDesc), sizeof(PosFromSeedsJob): sparse_align.hip asserts them
static const size_t kProblemBytes = 192, kCamBytes = 696, kJobBytes = 24;

static void print_block(int P, int C, int n, int S, int units)
{
  std::printf("case block problems=%d cams=%d n=%d shares=%d units=%d\n", P, C, n, S, units);
  AlignBlock b;
  for (int p = 0; p < P; ++p)
    for (int c = 0; c < C; ++c) {
      b.size_camera((size_t)n);
      if (units) b.size_seed_units((size_t)n);
    }
  b.lay_out((size_t)P * S, (size_t)P * C * S, kProblemBytes, kCamBytes);
  std::printf("desc %zu %zu %zu %zu\n", b.cams_off, b.ctl_off, b.bar_off, b.up_base);
  int n_jobs = 0;
  // as enqueue_align fills: a camera without features has no piece (its descriptor names the caller's arrays)
  for (int p = 0; p < P; ++p)
    for (int c = 0; c < C; ++c) {
      if (n == 0) continue;
      const size_t at = b.place_camera((size_t)n);
      const AlignCamColumns o((size_t)n);
      std::printf("cam %d %zu %zu %zu %zu %zu\n", p * C + c, at + o.px, at + o.f, at + o.pos, at + o.flags, o.stride);
      if (units) { std::printf("units %d %zu\n", p * C + c, b.place_seed_units((size_t)n)); ++n_jobs; }
      for (int s = 0; s < S; ++s) {
        const AlignShare sh(n, s, S);
        std::printf("share %d %d %zu %zu %zu %zu %zu\n", p * C + c, s, sh.n(), at + o.px + 16 * sh.lo, at + o.f + 24 * sh.lo, at + o.pos + 24 * sh.lo,
                    at + o.flags + sh.lo);
      }
    }
  if (n_jobs) std::printf("jobs %zu\n", b.place_job_table((size_t)n_jobs, kJobBytes));
  std::printf("total %zu %zu\n", b.reserve, b.used);
}

static int knob(const char* a, bool* set)
{
  *set = a[0] != 'u';
  return *set ? std::atoi(a) : 0;
}

static int replay(int argc, char** argv)
{
  if (argc < 4) return 2;
  bool overlap_set, side_set;
  const int overlap = knob(argv[2], &overlap_set), side = knob(argv[3], &side_set);
  AlignQueueState q;
  bool copy_stream = false, lane_stream = false;
  size_t cap[2] = { 0, 0 };   // the lanes' workspaces
  static const char* const kWait[] = { "free", "event", "drain" };
  for (int k = 4; k < argc; ++k) {
    const char* op = argv[k];
    if (op[0] == 'f') { q = align_drained(q); continue; }
    if (op[0] == 'j') { q.chain = false; q.lane1_pending = false; continue; }
    const bool batch = op[0] == 'b';
    size_t need = 1, bytes = 0;
    if (batch) {
      need = (size_t)std::strtoull(op + 1, nullptr, 10);
      if (const char* colon = std::strchr(op, ':')) bytes = (size_t)std::strtoull(colon + 1, nullptr, 10);
    }
    const bool grows = std::strchr(op, '!') != nullptr;
    // place in the queue, reserve
    const AlignBlockPlace bp = place_block(q);
    bool drained = bp.wait == kAlignBlockDrain;
    if (drained) q = align_drained(q);
    if (grows && align_busy(q)) { q = align_drained(q); drained = true; }
    if (op[0] == 'x') { std::printf("failed slot=%u wait=%s\n", bp.slot, kWait[bp.wait]); continue; }
    // the streams are made by the first launch that may use them, behind everything queued
    const bool side_kind = batch && align_side_wanted(side_set, side, bytes);
    if (side_kind && !copy_stream) { if (align_busy(q)) { q = align_drained(q); drained = true; } copy_stream = true; }
    const bool lane_kind = batch && align_overlap_wanted(overlap_set, overlap);
    if (lane_kind && !lane_stream) { if (align_busy(q)) { q = align_drained(q); drained = true; } lane_stream = true; }
    const bool ws_small[2] = { cap[0] && need > cap[0], cap[1] && need > cap[1] };
    const AlignLaunchPlan plan = place_launch(q, lane_kind, side_kind, ws_small, lane_stream && q.lane1_launches);
    if (plan.drain_first) {
      q = align_drained(q);
      drained = true;
      cap[plan.grow_lane] = need;
    }
    if (need > cap[plan.lane]) cap[plan.lane] = need;
    if (plan.join) { q.chain = false; q.lane1_pending = false; }
    q = commit_launch(q, plan, lane_kind);
    if (plan.record_kernel) note_kernel_recorded(q, plan);
    if (plan.record_lane1) note_lane1_recorded(q);
    std::printf("launch slot=%u lane=%d overlapped=%d side=%d wait=%s drained=%d\n", plan.slot, plan.lane, (int)plan.overlapped, (int)plan.side,
                kWait[bp.wait], (int)drained);
    if (op[0] == 'e') q = align_drained(q);
  }
  std::printf("end slot=%u lane1_launches=%llu side_launches=%llu\n", q.desc_slot, q.lane1_launches, q.side_launches);
  return 0;
}

int main(int argc, char** argv)
{
  if (argc > 1 && !std::strcmp(argv[1], "queue")) return replay(argc, argv);
  const int ns[] = { 0, 1, 15, 16, 17, 63, 64, 65 };
  const int problems[] = { 1, 3, 7 };
  for (int n : ns) for (int C = 1; C <= 2; ++C) for (int P : problems) for (int S = 1; S <= 3; S += 2) for (int units = 0; units < 2; ++units)
    print_block(P, C, n, S, units);
  const int feats[] = { 0, 1, 340, 341 };
  for (int f : feats) {
    const AlignWorkspace ws((size_t)f);
    std::printf("case workspace feat=%d\nws %zu %zu %zu %zu %zu\n", f, ws.slots, ws.wpk_off, ws.wsel_off, ws.wvis_off, ws.bytes);
  }
  return 0;
}
