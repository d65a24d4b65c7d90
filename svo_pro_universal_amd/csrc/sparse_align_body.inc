// sparse_align_body.inc -- the body of the resident alignment kernel, as TEXT: sparse_align.hip includes it into
// sparse_align_kernel<P, NT, ILLUM, CLUSTER, ROBUST, LPP, LAT, RIG> (Cam = CamModel) and into
// sparse_align_wide_kernel<P, ILLUM, ROBUST> (Cam = CamModelWide; NT = 512, CLUSTER = false, LPP = 1, LAT = RIG = false).
// In scope where it is included: Cam, P, NT, ILLUM, CLUSTER, ROBUST, LPP, LAT, RIG and the kernel's argument `a`.
// Text and not a __device__ function template on purpose: behind a function (always inlined, argument by reference, by
// restrict reference or by value alike) the compiler's passes in front of the inliner see another function than the kernel they
// saw before, and 16 of the 80 narrow kernels came out with other spill counts (33 -> 31, 60 -> 62, ...).  Included, every narrow
// kernel keeps its registers, spills and LDS (tests/test_kernel_resources_align_wide_cpu.py).
  static_assert(!LAT || (NT == 256 && !CLUSTER && LPP == 1), "latency build: the 256-thread lane-per-patch geometry");
  static_assert(!RIG || (!CLUSTER && LPP == 1 && (LAT || NT == 512)), "rig build: the two lane-per-patch geometries of small launches");
  static_assert(LPP == 1 || (!CLUSTER && NT == 512 && LPP <= P), "rows geometry: 512 threads, no cluster mode");
  static_assert(NT == 128 || NT == 256 || NT == 512, "workgroups of 128, 256 or 512 threads");
  static_assert(NT != 128 || (!CLUSTER && !LAT && !RIG && LPP == 1), "128 threads: the batch geometry only");
  // The arm that turns the rows of a rig's cameras >= 1 into camera 0's frame (jac_rows_cam): a wave-uniform branch in the patch loop of
  // every build but the 128-thread one, which the host gives single-camera launches only (decide_geometry).  The 256-thread batch build
  // serves launches with and without rigs with ONE kernel: a problem's result must be the same bits whatever else shares its launch
  // (AlignGeometry), and two instantiations of the same source do not round alike.
  constexpr bool kMultiCam = NT != 128;
  constexpr bool ROWS = LPP > 1;
  constexpr int D = ILLUM ? 8 : 6;
  constexpr int NACC = AccLayout<D>::NACC;
  constexpr int NW = NT / 64;

  // LDS-DMA staging of the workspace rows (accumulate_camera_staged) in the batch geometry; the wide
  // geometries keep their LDS for finer image levels and read the workspace with ordinary loads
  constexpr bool STAGED = (NT == 256 || NT == 128) && !ROWS;
  // the levels' images through registers in the BATCH geometry only (stage_item_list): a workgroup there has a second one beside it on its compute
  // unit to fill the wait; the small-launch geometries keep the LDS-DMA requests, whose flight overlaps the problem's base phase (measured, one
  // 180-patch problem: 27.6 us outside the iterations with LDS-DMA, 31.3 with the blocking copy)
  constexpr bool kStageRegs = (NT == 256 || NT == 128) && !LAT && !CLUSTER && !ROWS;
  // Half-level residency: a level whose pair of images does not fit the image area while ONE of them does runs with that one in
  // LDS and the other from global memory.  The 128-thread build only: its 23 KB hold levels 4 and 3 of a 640x480 pair and one
  // image of level 2; the wider builds hold all of level 2 and not even one image of level 1.
  constexpr bool kHalfLevel = NT == 128;
  // The resident one is the reference image (7 rows per 4x4 patch against the current image's 5; measured against the other
  // choice: no difference, profiles/r09_align_wg128_ab.txt).
  extern __shared__ __align__(16) unsigned char lds_img[];
  __shared__ __align__(16) double s_stage[STAGED ? NW * kStageDoubles : 2];
  __shared__ double s_jc[SVOH_MAX_CAMS][kJacConsts];   // per-camera constants of the camera-frame rows and of the pass's rotation (kJacConsts)
  __shared__ int s_lvl_off[SVOH_MAX_LEVELS];           // where the level's images start in lds_img; -1: not resident
  __shared__ double s_red[NW][NACC];
  static_assert(NACC <= 45, "g_sum is sized for the 8-parameter case");
  __shared__ double s_x[kXchgStride];   // cluster mode: the block handed to cluster_sum
  __shared__ int s_cluster_ok;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  __shared__ int s_pbi;
  __shared__ StageItem s_stage_items[kMaxStageItems];   // the images of the problem's resident levels (stage_item_list)
  // Persistent workgroups: the grid is sized to what is resident at once and every
  // workgroup pulls the next problem index from a queue head, so problems that need
  // more Gauss-Newton iterations do not leave CUs idle at the end of the launch.
  // (a clustered problem's shares placed on one XCD by block index, and the problem index taken from the block index when the grid
  // has a workgroup per problem: both tried, both lost -- HISTORY.md round 5, profiles/r05_align_cluster_xcd_ab.txt, r05_align_one_each_ab.txt)
  for (;;) {
  __syncthreads();  // everyone is done with the previous problem's shared state
  if (tid == 0) s_pbi = atomicAdd(a.queue, 1);
  __syncthreads();
  const int pbi = s_pbi;
  if (pbi >= a.n_problems) break;
#ifdef SVOH_TEST_HOOKS
  if (CLUSTER && a.cluster_test_absent && pbi % a.cluster == 1) continue;   // a partner that never arrives
#endif
  const DevProblemDesc& pb = a.problems[pbi];
  const DevCamDesc* cams = a.cams + pb.cam_begin;
  const int n_cams = pb.n_cams;
  const svoh_align_options& opt = a.opt;
  const bool eval_mode = a.eval_level >= 0;
  const int level_hi = eval_mode ? a.eval_level : opt.max_level;
  const int level_lo = eval_mode ? a.eval_level : opt.min_level;
  // LDS bytes of a level's images (all cameras), and their copy into lds_img + off (requests only: no wait)
  auto level_bytes = [&](int l) {
    int need = 0;
    for (int c = 0; c < n_cams; ++c) {
      need += ((cams[c].ref[l].w * cams[c].ref[l].h + 15) & ~15);
      need += ((cams[c].cur[l].w * cams[c].cur[l].h + 15) & ~15);
    }
    return need;
  };
  auto stage_level = [&](int l, int off) {
    for (int c = 0; c < n_cams; ++c) {
      const int off_cur = off + ((cams[c].ref[l].w * cams[c].ref[l].h + 15) & ~15);
      stage_image_pair<NT, kStageRegs>(lds_img + off, cams[c].ref[l], lds_img + off_cur, cams[c].cur[l], tid);
      off = off_cur + ((cams[c].cur[l].w * cams[c].cur[l].h + 15) & ~15);
    }
  };

  SVOH_STAMP_DECL
  SVOH_STAMP_START();
  // The images of the coarse levels are requested NOW, for the problem's whole life, from the coarsest level down
  // as long as they fit side by side (640x480: levels 4, 3, 2 = 50 400 bytes): their way from HBM overlaps the base
  // phase instead of standing in front of every level's first iteration (three exposed copies per problem before:
  // 6 % of a workgroup's life).  A finer level that fits only by itself is staged when its turn comes, over them.
  {
    // (uniform) which levels stay resident, and the table of their images; the list form wants images it can take in 16-byte pieces
    int off = 0, n_items = 0, total16 = 0;
    bool room = true, list_ok = kStageRegs;
    for (int l = level_hi; l >= level_lo; --l) {
      const int need = level_bytes(l);
      room = room && off + need <= a.lds_img_bytes;
      if (!room) continue;
      for (int c = 0; c < n_cams; ++c)
        for (int h = 0; h < 2; ++h) {
          const DevImage& im = h ? cams[c].cur[l] : cams[c].ref[l];
          list_ok = list_ok && n_items < kMaxStageItems && im.pitch == im.w && (reinterpret_cast<uintptr_t>(im.data) & 15) == 0;
          ++n_items;
        }
      off += need;
    }
    off = 0; room = true; n_items = 0;
    for (int l = level_hi; l >= level_lo; --l) {
      const int need = level_bytes(l);
      room = room && off + need <= a.lds_img_bytes;
      if (room) {
        if (!list_ok) stage_level(l, off);
        else if (tid == 0) {
          int o = off;
          for (int c = 0; c < n_cams; ++c)
            for (int h = 0; h < 2; ++h) {
              const DevImage& im = h ? cams[c].cur[l] : cams[c].ref[l];
              const int bytes = im.w * im.h;
              s_stage_items[n_items] = StageItem{ im.data, o, total16, bytes, 0 };
              ++n_items; total16 += bytes >> 4; o += (bytes + 15) & ~15;
            }
        } else {
          for (int c = 0; c < n_cams; ++c)
            for (int h = 0; h < 2; ++h) { const DevImage& im = h ? cams[c].cur[l] : cams[c].ref[l]; ++n_items; total16 += (im.w * im.h) >> 4; }
        }
        if (tid == 0) s_lvl_off[l] = off;
        off += need;
      }
      else if (tid == 0) s_lvl_off[l] = -1;
    }
    if (list_ok && n_items) {
      __syncthreads();   // the table is written
      stage_item_list<NT>(lds_img, s_stage_items, n_items, total16, tid);
    }
  }
  if (tid == 0) {
    g_state.T = load_rigid(pb.T_init);
    g_state.Told = g_state.T;
    g_state.alpha = pb.alpha_init; g_state.beta = pb.beta_init;
    if (a.ext_state) {
      g_state.T = load_rigid(a.ext_state->T_icur_iref);
      g_state.Told = g_state.T;
      g_state.alpha = a.ext_state->alpha; g_state.beta = a.ext_state->beta;
    }
    g_state.alpha_old = g_state.alpha; g_state.beta_old = g_state.beta;
    g_state.stop = 0; g_state.level_done = 0; g_state.nsel = 0; g_state.status = 0; g_state.patch_iters = 0;
    for (int k = 0; k < 8; ++k) g_state.I_prior[k] = 0.0;
    g_nvis = 0;
    g_state.prior = pb.prior;
    for (int c = 0; c < n_cams; ++c) {
      g_state.cam_cur_T_cam_imu[c] = load_rigid(cams[c].cur_T_cam_imu);
      g_state.cam_ref_T_imu_cam[c] = load_rigid(cams[c].ref_T_imu_cam);
      // the constants of jac_rows_cam: R_imu_cam, tau = R_imu_cam^T t_imu_cam and, behind camera 0, what takes the camera's rows to camera 0's frame
      double* jc = s_jc[c];
      to_matrix(g_state.cam_ref_T_imu_cam[c].q, jc);
      const Vec3 t = g_state.cam_ref_T_imu_cam[c].t;
      for (int k = 0; k < 3; ++k) jc[9 + k] = jc[k] * t.x + jc[3 + k] * t.y + jc[6 + k] * t.z;
      if (kMultiCam && c > 0)
        for (int i = 0; i < 3; ++i)
          for (int j = 0; j < 3; ++j) jc[12 + 3 * i + j] = s_jc[0][i] * jc[j] + s_jc[0][3 + i] * jc[3 + j] + s_jc[0][6 + i] * jc[6 + j];
    }
#ifdef SVOH_PHASE_STAMPS
    for (int k = 0; k < 4; ++k) g_state.dbg[k] = 0;
    for (int k = 0; k < 8; ++k) g_state.dbg2[k] = 0;
#endif
    for (int l = 0; l < SVOH_MAX_LEVELS; ++l) { g_state.lvl_iters[l] = 0; g_state.lvl_n_meas[l] = 0; g_state.lvl_chi2[l] = 0.0; }
  }
  __syncthreads();

  WsView ws = { a.wpk, a.slots, 0 };
  if constexpr (NT == 512) {
    if (a.ws_lds_bytes > 0) {   // this problem's rows (all cameras: consecutive slots from cams[0].feat_off on) in LDS
      int n_local = 0;
      for (int c = 0; c < n_cams; ++c) n_local += cams[c].n_features;
      if (n_local * kWsPairs * 16 <= a.ws_lds_bytes) {   // (the host sized the area for the launch's largest problem)
        ws.base = reinterpret_cast<double*>(lds_img + a.lds_img_bytes);
        ws.slots = n_local;
        ws.first = cams[0].feat_off;
      }
    }
  }
  // ---- a-3 extractFeaturesSubset + a-4 precomputeBaseCaches (depth, xyz_ref) ----
  {
    int my_sel = 0;
    const int patch_size_wb = P + 2;
    const double scale = 1.0f / (1 << opt.max_level);
    const double patch_center_wb = (patch_size_wb - 1) / 2.0f;
    for (int c = 0; c < n_cams; ++c) {
      const DevCamDesc& cd = cams[c];
      const int rows_minus_two = cd.ref[opt.max_level].h - 2;
      const int cols_minus_two = cd.ref[opt.max_level].w - 2;
      // all of a feature's inputs are requested together (they are independent; behind the selection test each
      // would be its own round trip to memory), and one feature ahead
      struct FeatIn { double pu, pv, pwx, pwy, pwz, fx, fy, fz; unsigned flag; };
      auto request = [&](int k, FeatIn& o) {
        o.flag = cd.flags[k];
        o.pu = cd.px[2 * k]; o.pv = cd.px[2 * k + 1];
        o.pwx = cd.pos_world[3 * k + 0]; o.pwy = cd.pos_world[3 * k + 1]; o.pwz = cd.pos_world[3 * k + 2];
        o.fx = cd.f[3 * k + 0]; o.fy = cd.f[3 * k + 1]; o.fz = cd.f[3 * k + 2];
      };
      // kBaseDepth features per thread are requested together and then worked off: their inputs come cold from HBM
      // (65 bytes per feature, read once), and the vector-memory counter is in order -- with one feature requested ahead
      // every trip waited for the PREVIOUS trip's stores as well (round 4 stamps: 99 K cycles per 2000-feature problem,
      // 12 K per trip: 9 % of a workgroup's life in the batch)
      // (128 threads: eight, so that a 2000-feature problem is two trips there as well.  Six pairs of the headline, eight against four:
      // 3.3243 - 3.3411 ms per step in five runs and ONE at 3.4418, against 3.3175 - 3.3762; medians 3.3365 / 3.3527, 0.5 %: inside the
      // spread, no gain shown -- profiles/r09_align_wg128_ab.txt.  Kept for the equal number of trips, and because the committed
      // kernels' own A/B was taken with it)
      constexpr int kBaseDepth = NT == 128 ? 8 : 4;
      for (int i0 = tid; i0 < cd.n_features; i0 += kBaseDepth * NT) {
        FeatIn in[kBaseDepth];
#pragma unroll
        for (int k = 0; k < kBaseDepth; ++k) {
          in[k] = FeatIn{ 0, 0, 0, 0, 0, 0, 0, 0, 0u };
          if (i0 + k * NT < cd.n_features) request(i0 + k * NT, in[k]);
        }
#pragma unroll
        for (int k = 0; k < kBaseDepth; ++k) {
          const int i = i0 + k * NT;
          if (i >= cd.n_features) break;
          const int gi = cd.feat_off + i;
          bool sel = in[k].flag != 0;
          const double pu = in[k].pu, pv = in[k].pv;
          const double pwx = in[k].pwx, pwy = in[k].pwy, pwz = in[k].pwz;
          const double fx_ = in[k].fx, fy_ = in[k].fy, fz_ = in[k].fz;
          if (sel) {
            const double u_tl = pu * scale - patch_center_wb;
            const double v_tl = pv * scale - patch_center_wb;
            const int u_tl_i = (int)floor(u_tl);
            const int v_tl_i = (int)floor(v_tl);
            // same test as sparse_img_align.cpp:221-225 with the constant moved to the right-hand side:
            // a wild pixel saturates the int conversion and `+ patch_size_wb` must not wrap around
            sel = !(u_tl_i < 0 || v_tl_i < 0 || u_tl_i >= cols_minus_two - patch_size_wb ||
                    v_tl_i >= rows_minus_two - patch_size_wb);
          }
          // the byte masks are what svoh_sparse_align_evaluate hands out; a run reads the row's state value alone.  (A lane's
          // vector-memory counter returns in order: in a run these two byte stores per feature were 16 of the 40 stores a
          // lane of a 2000-feature problem waits behind.)
          if (eval_mode) { a.wsel[gi] = sel ? 1 : 0; a.wvis[gi] = 0; }
          if (!sel) *reinterpret_cast<double2*>(ws_pair(ws, 2, gi)) = make_double2(0.0, 0.0);
          if (sel) {
            const double dx = pwx - cd.ref_pos[0];
            const double dy = pwy - cd.ref_pos[1];
            const double dz = pwz - cd.ref_pos[2];
            const double depth = sqrt(dx * dx + dy * dy + dz * dz);
            const Vec3 X = { fx_ * depth, fy_ * depth, fz_ * depth };
            *reinterpret_cast<double2*>(ws_pair(ws, 0, gi)) = make_double2(X.x, X.y);
            *reinterpret_cast<double2*>(ws_pair(ws, 1, gi)) = make_double2(X.z, pu);
            *reinterpret_cast<double2*>(ws_pair(ws, 2, gi)) = make_double2(pv, 1.0);
            ++my_sel;
          }
        }
      }
    }
    if (my_sel) atomicAdd(&g_state.nsel, my_sel);
  }
  __syncthreads();
  SVOH_STAMP_ADD(0);
  constexpr bool cluster = CLUSTER;
  // cluster mode: descriptor pbi is share (pbi % G) of problem (pbi / G); share 0 reports the common result in
  // the problem's slot, the other shares write theirs behind the problems' slots
  const int c_prob = cluster ? pbi / a.cluster : pbi;
  const int c_share = cluster ? pbi % a.cluster : 0;
  const int res_idx = cluster ? (c_share == 0 ? c_prob : a.n_problems / a.cluster + pbi) : pbi;
  unsigned cluster_epoch = 0;
  bool cluster_failed = false;
  int n_sel = g_state.nsel;
  if (cluster) {   // the number of selected features of the whole problem, not of this share
    if (tid == 0) s_x[0] = (double)n_sel;
    __syncthreads();
    cluster_failed = !cluster_sum<NT>(a, c_prob, c_share, cluster_epoch, s_x, 1, tid, &s_cluster_ok);
    n_sel = cluster_failed ? 0 : (int)s_x[0];
    __syncthreads();
  }
  if (n_sel == 0) {
    if (tid == 0) {
      svoh_align_result& r = a.results[res_idx];
      r.status = cluster_failed ? 3 : 1; r.n_fts_to_track = 0;
      store_rigid(g_state.T, r.T_icur_iref);
      r.alpha = g_state.alpha; r.beta = g_state.beta;
      r.n_patch_iters = 0;
      for (int l = 0; l < SVOH_MAX_LEVELS; ++l) { r.iters[l] = 0; r.n_meas[l] = 0; r.chi2[l] = 0.0; }
      if (eval_mode) for (int k = 0; k < 74; ++k) a.eval_out[74 * pbi + k] = 0.0;
    }
    SVOH_STAMP_FLUSH();
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): no image request of this problem lands in the next one's
    continue;
  }
  const bool est_alpha = opt.estimate_illumination_gain != 0;
  const bool est_beta = opt.estimate_illumination_offset != 0;
  constexpr bool robust = ROBUST;
  const bool dist_jac = opt.use_distortion_jacobian != 0;
  const float weight_scale = (float)opt.weight_scale;

  // cameras side by side (run_cameras): when the patches of all cameras fit the workgroup together, wave after wave
  constexpr int kLanesPerPatch = ROWS ? LPP : 1;
  bool side_by_side = false;
  if (RIG && n_cams >= 2) {
    int lanes_needed = 0;
    for (int c = 0; c < n_cams; ++c) lanes_needed += (cams[c].n_features * kLanesPerPatch + 63) & ~63;
    side_by_side = lanes_needed <= NT;
  }

  for (int level = level_hi; level >= level_lo; --level) {
    const double scale = 1.0f / (1 << level);
    // ---- the level's images: resident since the problem's start, staged now, or read from global memory ----
    int lvl_off = s_lvl_off[level];
    bool in_lds = lvl_off >= 0;
    if (!in_lds && level_bytes(level) <= a.lds_img_bytes) {
      // not resident (the coarser levels took the room) but it fits by itself: over the levels that are done
      __syncthreads();  // their readers are done with lds_img
      stage_level(level, 0);
      lvl_off = 0;
      in_lds = true;
    }
    // ... and one whose pair does not fit while one of its images does (one camera): that image alone, over the levels that
    // are done; the passes read the other from global memory
    bool half_lds = false;
    if constexpr (kHalfLevel) {
      if (!in_lds && n_cams == 1) {
        const DevImage& him = cams[0].ref[level];
        if (((him.w * him.h + 15) & ~15) <= a.lds_img_bytes) {
          __syncthreads();   // the finished levels' readers are done with lds_img
          DevImage none = him;   // (the pair's copy with an empty second image: through registers where the pairs go that way)
          none.w = none.h = none.pitch = 0;
          stage_image_pair<NT, kStageRegs>(lds_img, him, lds_img, none, tid);
          half_lds = true;
        }
      }
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): this thread's image requests (issued here or at the problem's start) have landed
    __syncthreads();
    if (tid == 0) {
      g_state.level_done = 0;
      for (int c = 0; c < n_cams; ++c)
        g_state.Tcr[c] = mul(mul(g_state.cam_cur_T_cam_imu[c], g_state.T), g_state.cam_ref_T_imu_cam[c]);
      g_state.alpha_f = (float)g_state.alpha; g_state.beta_f = (float)g_state.beta;
      g_state.Told = g_state.T; g_state.alpha_old = g_state.alpha; g_state.beta_old = g_state.beta;  // old_state = state (hpp:45)
    }
    __syncthreads();
    SVOH_STAMP_ADD(1);

    for (int iter = 0; iter < opt.max_iter; ++iter) {
      const double one_plus_alpha = uniform_f64(1.0 + (double)g_state.alpha_f);
      const double beta_d = uniform_f64((double)g_state.beta_f);
      // Without robust weights the Hessian of a level only depends on which patches are visible (the Jacobians
      // are the reference patch's: inverse compositional), so after the level's first iteration a pass computes
      // the gradient and chi2 only and the solver reuses the level's factorisation.  A pass that finds a patch
      // whose visibility differs from the last full pass is thrown away and repeated in full: the numbers are
      // those of recomputing the Hessian every iteration, as the reference does.
      bool light = !eval_mode && !robust && iter > 0;
      for (;;) {
        int nvis = 0, changed = 0;
        auto run_cameras = [&](auto gonly_tag, auto& acc_ref) {
          constexpr bool G = decltype(gonly_tag)::value;
          int off = lvl_off;
          // A rig of several cameras whose patches fit the workgroup together: the cameras run SIDE BY SIDE, camera c on
          // the waves behind camera c-1's (whole waves: the choice is wave-uniform), instead of one after the other on the
          // same few waves -- a stereo bundle of 2 x 160 patches is one round of 3 + 3 waves (spread over the four SIMDs
          // by the hardware's wave placement), not two rounds of 3.  The normal equations are the sum over the cameras
          // either way (sparse_img_align.cpp:138-154); a lane's partial sum now holds one camera's patches, so sums differ
          // in order only.  Not when the patches do not fit: the cameras then take turns with the whole workgroup.
          // (side_by_side: decided once per problem, above the level loop)
          int cam_base = 0;
          for (int c = 0; c < n_cams; ++c) {
            const DevCamDesc& cdg = cams[c];
            CamPass cd;
            cd.cam = cdg.cam; cd.n_features = cdg.n_features; cd.feat_off = cdg.feat_off;
            const DevImage& rim = cdg.ref[level];
            const DevImage& cim = cdg.cur[level];
            const Rigid Tcr = uniform_rigid(g_state.Tcr[c]);
            unsigned cam_stride = NT, cam_t = (unsigned)tid;
            if (RIG && side_by_side) {   // (uniform)
              const int cam_width = (cd.n_features * kLanesPerPatch + 63) & ~63;
              cam_stride = (unsigned)cam_width;
              cam_t = (unsigned)(tid - cam_base);
              cam_base += cam_width;
            }
            if (kHalfLevel && half_lds) {
              if constexpr (kHalfLevel) {   // (the batch geometry: one camera, the whole workgroup)
                ImgView<true> ref;
                ImgView<false> cur;
                ref.p = (const __attribute__((address_space(3))) uint8_t*)lds_img; ref.pitch = rim.w;
                cur.p = cim.data; cur.pitch = cim.pitch;
                accumulate_camera_staged<Cam, P, D, NT, true, kMultiCam, G, ROBUST, false>(a, cd, ref, cur, cim.w, cim.h, Tcr, scale, one_plus_alpha, beta_d,
                                                                                   est_alpha, est_beta, robust, dist_jac, weight_scale, (int)cam_t,
                                                                                   s_stage + wave * kStageDoubles, s_jc[c], c > 0, acc_ref, nvis, changed, (int)cam_stride);
              }
            } else if (in_lds) {
              ImgView<true> ref, cur;
              ref.p = (const __attribute__((address_space(3))) uint8_t*)(lds_img + off); ref.pitch = rim.w;
              off += ((rim.w * rim.h + 15) & ~15);
              cur.p = (const __attribute__((address_space(3))) uint8_t*)(lds_img + off); cur.pitch = cim.w;
              off += ((cim.w * cim.h + 15) & ~15);
              if constexpr (ROWS) {
                if (!RIG || cam_t < cam_stride)
                  accumulate_camera_rows<Cam, P, (ROWS ? LPP : 2), D, NT, true, kMultiCam, G, ROBUST>(a, ws, cd, ref, cur, cim.w, cim.h, Tcr, scale, one_plus_alpha, beta_d,
                                                                            est_alpha, est_beta, robust, dist_jac, weight_scale, (int)cam_t, s_jc[c], c > 0,
                                                                            acc_ref, nvis, changed, (int)cam_stride);
              } else if constexpr (STAGED) {
                if (!RIG || cam_t < cam_stride)
                  accumulate_camera_staged<Cam, P, D, NT, true, kMultiCam, G, ROBUST>(a, cd, ref, cur, cim.w, cim.h, Tcr, scale, one_plus_alpha, beta_d,
                                                            est_alpha, est_beta, robust, dist_jac, weight_scale, (int)cam_t,
                                                            s_stage + wave * kStageDoubles, s_jc[c], c > 0, acc_ref, nvis, changed, (int)cam_stride);
              }
              else if (!RIG || cam_t < cam_stride)   // (unsigned: the lanes of the cameras in front are "negative")
                accumulate_camera<Cam, P, D, NT, true, kMultiCam, G, ROBUST>(a, ws, cd, ref, cur, cim.w, cim.h, Tcr, scale, one_plus_alpha, beta_d,
                                                     est_alpha, est_beta, robust, dist_jac, weight_scale, (int)cam_t, s_jc[c], c > 0, acc_ref,
                                                     nvis, changed, (int)cam_stride);
            } else {
              ImgView<false> ref, cur;
              ref.p = rim.data; ref.pitch = rim.pitch;
              cur.p = cim.data; cur.pitch = cim.pitch;
              if constexpr (ROWS) {
                if (!RIG || cam_t < cam_stride)
                  accumulate_camera_rows<Cam, P, (ROWS ? LPP : 2), D, NT, false, kMultiCam, G, ROBUST>(a, ws, cd, ref, cur, cim.w, cim.h, Tcr, scale, one_plus_alpha, beta_d,
                                                                             est_alpha, est_beta, robust, dist_jac, weight_scale, (int)cam_t, s_jc[c], c > 0,
                                                                             acc_ref, nvis, changed, (int)cam_stride);
              } else if constexpr (STAGED) {
                if (!RIG || cam_t < cam_stride)
                  accumulate_camera_staged<Cam, P, D, NT, false, kMultiCam, G, ROBUST>(a, cd, ref, cur, cim.w, cim.h, Tcr, scale, one_plus_alpha, beta_d,
                                                             est_alpha, est_beta, robust, dist_jac, weight_scale, (int)cam_t,
                                                             s_stage + wave * kStageDoubles, s_jc[c], c > 0, acc_ref, nvis, changed, (int)cam_stride);
              }
              else if (!RIG || cam_t < cam_stride)   // (unsigned: the lanes of the cameras in front are "negative")
                accumulate_camera<Cam, P, D, NT, false, kMultiCam, G, ROBUST>(a, ws, cd, ref, cur, cim.w, cim.h, Tcr, scale, one_plus_alpha, beta_d,
                                                      est_alpha, est_beta, robust, dist_jac, weight_scale, (int)cam_t, s_jc[c], c > 0, acc_ref,
                                                      nvis, changed, (int)cam_stride);
            }
          }
        };
        if (light) {
          double accg[D + 1];
#pragma unroll
          for (int k = 0; k < D + 1; ++k) accg[k] = 0.0;
          SVOH_OUTER_STAMP_BEGIN();
          run_cameras(std::true_type(), accg);
          SVOH_OUTER_STAMP(5);   // includes the pieces 0..4 counted inside
          // (the vote carried by the reduction's barrier, one barrier less: tried, lost -- HISTORY.md round 5, profiles/r05_align_desc_vote_ab.txt)
          const int changed_here = __syncthreads_or(changed);
          SVOH_OUTER_STAMP(6);
          if (changed_here && !cluster) {   // visibility moved: this iteration in full
            SVOH_STAMP_COUNT(5);
            light = false;
            continue;
          }
          SVOH_STAMP_COUNT(6);
          SVOH_STAMP_ADD(2);
          {
            int ridx;
            bool rvalid;
            wave_reduce_scatter<D + 1>(accg, lane, ridx, rvalid);
            if (rvalid) s_red[wave][ridx] = accg[0];
          }
          nvis = wave_sum_i32_dpp(nvis);
          if (lane == 0) atomicAdd(&g_nvis, nvis);
          __syncthreads();
          // gradient and chi2 only: g_sum[0 .. NH) still holds the level's (rotated) Hessian
          rotate_sums<D, NW, NACC, true>((LdsConstDoubles)&s_red[0][0], (LdsConstDoubles)s_jc[0], tid);
          __syncthreads();
          if (cluster) {   // gradient, chi2, visible count and the visibility vote of all shares
            if (tid < D + 1) s_x[tid] = g_sum[AccLayout<D>::NH + tid];
            if (tid == 0) { s_x[D + 1] = (double)g_nvis; s_x[D + 2] = changed_here ? 1.0 : 0.0; }
            __syncthreads();
            if (!cluster_sum<NT>(a, c_prob, c_share, cluster_epoch, s_x, D + 3, tid, &s_cluster_ok)) { cluster_failed = true; break; }
            const bool changed_anywhere = s_x[D + 2] != 0.0;
            __syncthreads();
            if (changed_anywhere) {
              if (tid == 0) g_nvis = 0;
              __syncthreads();
              light = false;
              continue;
            }
            if (tid < D + 1) g_sum[AccLayout<D>::NH + tid] = s_x[tid];
            if (tid == 0) g_nvis = (int)s_x[D + 1];
            __syncthreads();
          }
        } else {
          double acc[NACC];
#pragma unroll
          for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
          run_cameras(std::false_type(), acc);
          SVOH_STAMP_ADD(2);
          // ---- reduce: butterfly reduce-scatter per wave, then across waves through LDS ----
          {
            int ridx;
            bool rvalid;
            wave_reduce_scatter<NACC>(acc, lane, ridx, rvalid);
            if (rvalid) s_red[wave][ridx] = acc[0];
          }
          nvis = wave_sum_i32_dpp(nvis);
          if (lane == 0) atomicAdd(&g_nvis, nvis);
          __syncthreads();
          rotate_sums<D, NW, NACC, false>((LdsConstDoubles)&s_red[0][0], (LdsConstDoubles)s_jc[0], tid);
          __syncthreads();
          if (cluster) {
            if (tid < NACC) s_x[tid] = g_sum[tid];
            if (tid == 0) s_x[NACC] = (double)g_nvis;
            __syncthreads();
            if (!cluster_sum<NT>(a, c_prob, c_share, cluster_epoch, s_x, NACC + 1, tid, &s_cluster_ok)) { cluster_failed = true; break; }
            if (tid < NACC) g_sum[tid] = s_x[tid];
            if (tid == 0) g_nvis = (int)s_x[NACC];
            __syncthreads();
          }
        }
        break;
      }
      if (cluster_failed) break;

      SVOH_STAMP_ADD(3);
      // ---- serial part: prior, pivoted LDL^T (or the level's factor again), SE3 update, convergence ----
      if (eval_mode) { if (tid == 0) gn_serial_step<P, D, ILLUM>(a, pb, cams, n_cams, res_idx, level, iter, eval_mode, light); }
      else if (tid < 64) {
        // the step is its workgroup's critical path (three waves wait at the barrier behind it): it goes ahead of the
        // other workgroup's pass waves on its SIMD
        __builtin_amdgcn_s_setprio(3);
        gn_wave_step<P, D, ILLUM>(a, n_cams, level, iter, light, tid);
        __builtin_amdgcn_s_setprio(0);
      }
      __syncthreads();
      SVOH_STAMP_ADD(4);
      if (g_state.level_done) break;
    }
    if (cluster_failed) break;
  }

  if (tid == 0) {
    svoh_align_result& r = a.results[res_idx];
    r.status = cluster_failed ? 3 : g_state.status;   // 3: a workgroup of the cluster never arrived (see cluster_sum)
    r.n_fts_to_track = n_sel;
    store_rigid(g_state.T, r.T_icur_iref);
    r.alpha = g_state.alpha; r.beta = g_state.beta;
    r.n_patch_iters = g_state.patch_iters;
    for (int l = 0; l < SVOH_MAX_LEVELS; ++l) { r.iters[l] = g_state.lvl_iters[l]; r.n_meas[l] = g_state.lvl_n_meas[l]; r.chi2[l] = g_state.lvl_chi2[l]; }
  }
  SVOH_STAMP_FLUSH();
  }  // next problem
