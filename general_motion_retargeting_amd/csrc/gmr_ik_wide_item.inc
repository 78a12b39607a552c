// gmr_ik_wide_item.inc -- one queue item of the throughput kernel: frames [t0, t1) of local stream `s` (global id `gs`)
// of one job.  Included, textually, inside the item loop of BOTH kernels of gmr_ik_wide.hip (`break` leaves that loop):
// the plain kernel, where the job's fields are kernel arguments, and the group kernel, where they are scalar loads from
// the job table.  One text, because the register allocation of this 7 000-instruction loop nest reacts to how the code
// is packaged (the same statements behind an inlined function boundary: 40 VGPRs spilled to scratch, -4 % frames/s),
// not only to what it computes.
//
// Names the including scope provides: img, D (type GMR_DIMS_T), max_iter, human_root, use0, use1, T, q0, human, len,
// flags, q_out, nsolve, status, tgt_out, err_out, Q, queued, s, gs, t0, stat, bounds, nq, prm, fstride, sm, lane, pr; and the
// macros GMR_T_END (frames at or beyond it are left to a later launch: T in the plain kernel), GMR_WINDOWED (the launch is one
// window of a stream's frames: its state is kept in Q.state for the next window; false in the plain kernel) and GMR_SCALE (the
// job's per-stream human scale tables, f64 [S][nhum], or null = the image's table; a literal null in the plain kernel); and
// GMR_FWIN, a literal: the instance applies the frame window (gmr_ik_wide_kernels.inc); and GMR_WGT, 0 or 1: the instance
// applies GMR_WEIGHT, the job's per-frame body weights (f64 [S][T][nhum], or null = every multiplier is 1; only
// ik_wide_group_w_kernel).  What the weights add stands behind #if GMR_WGT, so that the other instances compile the text they
// compiled without the feature.  The frame's row is indexed by t in the stream and read where it is used -- by the body lanes before
// the preprocessing, by the task lanes once per stage (L1 hits: the same 128 bytes) --, so queue items and later windows carry no
// state for it and no LDS holds it.
  // state that must start defined: the violation sets of the QP (double-buffered, cleared round by round)
  if (lane < 8) reinterpret_cast<unsigned long long*>(sm + LD.vset)[lane] = 0ull;
  {
    const double* qs = t0 == 0 ? q0 + (size_t)s * nq : q_out + ((size_t)s * T + t0 - 1) * nq;
    for (int i = lane; i < nq; i += 64) (sm + LD.q)[i] = qs[i];
  }
  wsync();
  hinge_sincos<GMR_DIMS_T>(D, sm, lane);
  wsync();
  fk_wide<GMR_DIMS_T>(D, sm, img, lane, pr, t0 > 0);

  const int Ts = len ? min(len[s], T) : T;
  const int Tw = min(Ts, GMR_T_END);                 // this launch's share of the stream
  const int t1 = queued ? min(t0 + Q.chunk, Tw) : Tw;
  const double* hs = human + (size_t)s * T * fstride;
  const double* scl = GMR_SCALE ? GMR_SCALE + (size_t)s * D.nhum : nullptr;
#if GMR_WGT
  const double* wstream = GMR_WEIGHT ? GMR_WEIGHT + (size_t)s * T * D.nhum : nullptr;
#endif
  double r0 = 0.0, r1 = 0.0;
  if (t0 < t1) {
    const double* nx = hs + (size_t)t0 * fstride;
    if (lane < (int)fstride) r0 = nx[lane];
    if (lane + 64 < (int)fstride) r1 = nx[lane + 64];
  }
  for (int t = t0; t < t1; t++) {
    if (lane < (int)fstride) (sm + LD.raw)[lane] = r0;
    if (lane + 64 < (int)fstride) (sm + LD.raw)[lane + 64] = r1;
    if (t + 1 < t1) {                                  // prefetch the next frame (nhuman * 7 <= 112 doubles)
      const double* nx = hs + (size_t)(t + 1) * fstride;
      if (lane < (int)fstride) r0 = nx[lane];
      if (lane + 64 < (int)fstride) r1 = nx[lane + 64];
    }
    wsync();
    // The frame window (gmr_solver_set_frame_velocity_limits): every solve of this frame keeps the hinges within fw of the
    // angle the frame starts from -- LDS q holds it here: the previous frame's result, q0, or the q_out row an earlier item
    // or window wrote.  Only in the instances with GMR_FWIN (gmr_ik_wide_kernels.inc); whether the frame is bounded is decided
    // where the window is applied (cvec_wide), from values the wavefront can re-load, so that this register pair is all the
    // window keeps alive across the frame.  Frame 0 of a stream is bounded only on the caller's word.
    const double th0 = (GMR_FWIN && lane >= 6 && lane < D.nv) ? (sm + LD.q)[7 + lane - 6] : 0.0;
    int ns0 = 0, ns1 = 0;
    const size_t f = (size_t)s * T + t;
#if GMR_WGT
    const double* wrow = wstream ? wstream + (size_t)t * D.nhum : nullptr;      // this frame's multipliers, by human body
#endif
    if (stat == GMR_STATUS_OK) {
#if GMR_WGT
      // a body whose multiplier is 0 is missing in this frame (the human root's row is always read: every body moves with it)
      const bool missing = wrow && lane < D.nhum && lane != human_root && wrow[lane] == 0.0;
      preprocess_wide<GMR_DIMS_T, true>(D, sm, img, scl, human_root, prm[4], flags, lane, pr, missing);
      if (tgt_out) {   // the poses handed to task.set_target (motion_retarget.py:117-136) = scaled_human_data
        if (!wrow) {
          for (int i = lane; i < (int)fstride; i += 64) tgt_out[f * fstride + i] = (sm + LD.tgt)[i];
        } else if (lane < D.nhum) {      // a body lane stores its own row: seven NaNs for a missing body, as for an absent one
          for (int r = 0; r < 7; r++) tgt_out[f * fstride + 7 * lane + r] = missing ? (double)NAN : (sm + LD.tgt)[7 * lane + r];
        }
      }
#else
      preprocess_wide<GMR_DIMS_T>(D, sm, img, scl, human_root, prm[4], flags, lane, pr);
      if (tgt_out)     // the poses handed to task.set_target (motion_retarget.py:117-136) = scaled_human_data
        for (int i = lane; i < (int)fstride; i += 64) tgt_out[f * fstride + i] = (sm + LD.tgt)[i];
#endif
      double last_E = -1.0;                          // the stage's last residual norm (at the current configuration)
      for (int stage = 0; stage < 2; stage++) {
        if (!(stage == 0 ? use0 : use1) || (flags & GMR_FLAG_EVAL_ONLY)) continue;
        const int K = D.K[stage];
        const uint32_t taskw = lane < K ? img_at<uint32_t>(img, IM.taski[stage])[lane] : 0u;
        // (same task list in both tables -- bit 1 of use1, gmr_ik_layout.h: the first stage's last evaluation is this
        //  stage's first, and its residuals and log-map terms are still in LDS for the Jl^-1 phase)
#if GMR_WGT
        const double mk = task_mult(wrow, taskw, K, lane);      // the multiplier of this lane's task (1 for a job without weights)
        const bool keep = mk != 0.0;
        double curr = (stage == 1 && (use1 & 2) && last_E >= 0.0) ? last_E : errors_wide<true>(sm, taskw, K, lane, pr, keep);
#else
        double curr = (stage == 1 && (use1 & 2) && last_E >= 0.0) ? last_E : errors_wide(sm, taskw, K, lane, pr);
#endif
        int nsol = 0, num_iter = 0;
        for (;;) {
#if GMR_WGT
          const double mu = jlog_wide<true>(sm, img, stage, K, prm[1], lane, pr, mk);
#else
          const double mu = jlog_wide(sm, img, stage, K, prm[1], lane, pr);
#endif
          const double diag = prm[0] + mu;
          PROF_BEGIN(pr);
          pairs_wide(sm, img, stage, D.P[stage], lane);
          wsync();
          PROF_END(pr, PH_PAIRS);
          PROF_BEGIN(pr);
          cvec_wide<GMR_DIMS_T>(D, sm, img, stage, prm[3], GMR_FWIN && (t > 0 || (flags & GMR_FLAG_FRAME_LIMIT_FIRST)), th0, lane);
          PROF_END(pr, PH_CVEC);
          PROF_BEGIN(pr);
          hacc_wide(sm, img, D.items[stage], D.ntrip[stage], diag, lane);
          wsync();
          PROF_END(pr, PH_HACC);
          PROF_COUNT(pr, PH_NSOLVE);
          PROF_COUNT(pr, PH_NFACT);
          const int rc = solve_rows<GMR_DIMS_T>(D, sm, img, lane, bounds, pr);
          if (rc != GMR_STATUS_OK) { stat = rc; break; }
          integrate_wide<GMR_DIMS_T>(D, sm, prm[5], lane, pr);
          fk_wide<GMR_DIMS_T>(D, sm, img, lane, pr);
#if GMR_WGT
          const double next = errors_wide<true>(sm, taskw, K, lane, pr, keep);
#else
          const double next = errors_wide(sm, taskw, K, lane, pr);
#endif
          last_E = next;
          nsol++;
          if (nsol > 1) num_iter++;
          if (!(curr - next > prm[2] && num_iter < max_iter)) break;
          curr = next;
        }
        if (stage == 0) ns0 = nsol; else ns1 = nsol;
        if (stat != GMR_STATUS_OK) break;
      }
    }
    if (err_out && stat == GMR_STATUS_OK) {
      // error1() / error2() of the reference (motion_retarget.py:188-200) at the configuration this frame ends with
      for (int stage = 0; stage < 2; stage++) {
        double E = 0.0;
        if (stage == 0 ? use0 : use1) {
          const int K = D.K[stage];
#if GMR_WGT
          const uint32_t taskw = lane < K ? img_at<uint32_t>(img, IM.taski[stage])[lane] : 0u;
          E = errors_wide<true>(sm, taskw, K, lane, pr, task_mult(wrow, taskw, K, lane) != 0.0);
#else
          E = errors_wide(sm, lane < K ? img_at<uint32_t>(img, IM.taski[stage])[lane] : 0u, K, lane, pr);
#endif
        }
        if (lane == 0) err_out[2 * f + stage] = E;
      }
    }
    for (int i = lane; i < nq; i += 64) q_out[f * nq + i] = (sm + LD.q)[i];
    if (lane == 0) { nsolve[2 * f] = ns0; nsolve[2 * f + 1] = ns1; }
    wsync();
  }
  if (!queued) {
    if (lane == 0) {
      if (!GMR_WINDOWED || t1 >= Ts) status[s] = stat;
      if (GMR_WINDOWED) Q.state[gs] = WideStreamState{bounds.lower, bounds.upper, t1, stat};
    }
    break;
  }
  if (t1 < Tw) {
    // hand the stream back: state, then (release) its ring entry.  The q_out rows of this chunk were stored by all
    // lanes; the fence is executed by the wavefront, so it covers them.
    if (lane == 0) Q.state[gs] = WideStreamState{bounds.lower, bounds.upper, t1, stat};
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    if (lane == 0) {
      const unsigned slot = __hip_atomic_fetch_add(&Q.hdr[1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&Q.ring[slot], (unsigned)gs + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
  } else if (lane == 0) {
    if (!GMR_WINDOWED || t1 >= Ts) status[s] = stat;
    if (GMR_WINDOWED) Q.state[gs] = WideStreamState{bounds.lower, bounds.upper, t1, stat};   // (the next window continues from here)
  }
  wsync();
