// band_forward_body.inc -- the body of band.hip's forward sweep kernel, included once per entry point (band.hip: the pair of a
// launch comes out of the launch's table, or -- a launch of one pair -- is the kernel's own argument).  GTNX_BAND_PAIR
// names it.  Not a translation unit of its own.
// (-DGTNX_FWD_SHIFT_ROWS=8: one shift per block of eight rows -- measured: the forward sweep 2.3 % faster (0.214 against
//  0.219 ms), emission gradients 2.2e-5 instead of 1.9e-5 from float64 and target-arc gradients 1.3e-4 instead of 8e-5
//  at C3; the accuracy is kept)
// (-DGTNX_FWD_IDLE_FROM=w, set by the including kernel: waves w and up have no role and only keep the barrier count;
//  not defined -- band.hip -- the workgroup is the eight waves of the two roles)
#ifndef GTNX_FWD_SHIFT_ROWS
#define GTNX_FWD_SHIFT_ROWS 4
#endif
  constexpr int RNk = K >= GTNX_FWD_SHIFT_ROWS ? GTNX_FWD_SHIFT_ROWS : (K >= 4 ? 4 : K);  // rows between shifts of a wave's running row
  constexpr int NP = K / RNk;          // shift periods per block
  // ticks a staged chunk is in flight: 8 rows ahead, and never less than two ticks -- with one (K = 8) a request had
  // ~1.5 us to come back and the landing wave waited another 1000 cycles for it every tick (band_bench_tm: land 1056)
  constexpr int D = 8 / K > GTNX_FWD_DEPTH ? 8 / K : GTNX_FWD_DEPTH;
  const BandPair P = GTNX_BAND_PAIR;
  const int T = P.T, C = P.C, NS = P.NS;
  extern __shared__ float lds[];
  const BandLds L = band_lds(C, K, NSmax, false);
  float* ering = lds + L.o_ering;
  const BandMisc M = band_misc<K>(lds, L);
  const int CS = L.CS;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool sweeper = wv < 4;
  const int l = threadIdx.x & 63;
  const int nblocks = (T + K - 1) / K;
  const int nticks = nblocks + 3;
  GTNX_TM_INIT(0);

  if (sweeper) {
    __builtin_amdgcn_s_setprio(1);  // the recursion is the critical path; the staging waves of the CU's other workgroup yield (2 %)
    // ------------------------------------------------------------------ the recursion: no global loads
    const int w = wv;
    const int m0 = threadIdx.x * NPL;
    NodeRegs<NPL> g;
    load_nodes<NPL, false>(P, m0, g);
    const bool writer = m0 < NS;
    float a[NPL];
#pragma unroll
    for (int j = 0; j < NPL; ++j) a[j] = g.start[j] ? 0.0f : NEGF;
    double off = 0.0;  // this wave's shift: true alpha = a + off
    // (a row's address is a uniform base that advances by the row stride + this lane's byte offset: no 64-bit lane
    //  arithmetic per row)
    const GTNX_G char* arow = reinterpret_cast<const GTNX_G char*>(P.alpha);
    const unsigned aoffb = unsigned(m0) * 4u;
    auto store_row = [&](const float* v) {
#pragma unroll
      for (int j = 0; j < NPL; ++j) *reinterpret_cast<GTNX_G float*>(const_cast<GTNX_G char*>(arow) + (aoffb + 4u * j)) = v[j];
    };
    if (writer) store_row(a);
    // pipeline position s = w: this wave publishes into region s + 1 and reads region s (0: constants)
    float* bnd_own = M.bndr + (w + 1) * 4 * K * 2;
    const float* bnd_prev = M.bndr + w * 4 * K * 2;
    double* off_own = M.offr + (w + 1) * 16;
    const double* off_prev = M.offr + w * 16;
    if (threadIdx.x < 8 * K) M.bndr[threadIdx.x] = NEGF;
    if (threadIdx.x < 16) M.offr[threadIdx.x] = 0.0;
    if (l == 0) {
      P.aoff[1 + w] = 0.0;
      off_own[0] = 0.0;
    }
    if (NPL == 1) {
      if (l >= 62) bnd_own[63 - l] = a[0];
    } else if (l == 63) {
      bnd_own[0] = a[NPL - 1];
      bnd_own[1] = a[0];
    }
    lds_barrier();
    // (ring positions as counters, not as divisions by 5: band_backward_body.inc)
    int bm5 = ((-w % NBE) + NBE) % NBE;  // beta % NBE
    for (int tau = 0; tau < nticks; ++tau, bm5 = bm5 + 1 == NBE ? 0 : bm5 + 1) {
      GTNX_TM(0);
      const int beta = tau - w;
      // (every block but the last holds K rows: that one, the common one, is compiled without the per-row tests --
      //  a wave issues one instruction per four cycles whatever its kind, and the scalar compare / branch / exec-mask
      //  instructions of `i < rows` were a sixth of the 583 a tick of eight rows took)
      auto block = [&](auto full_tag) {
        constexpr bool FULL = decltype(full_tag)::value;
        const int t0 = beta * K, rows = FULL ? K : min(K, T - t0);
        const float* eb = ering + bm5 * K * CS;
        float ev[K][NPL], bv1[K], bv2[K];
        double offp[NP + 1];
#pragma unroll
        for (int i = 0; i < K; ++i) {
#pragma unroll
#ifdef GTNX_EXP_NOCONFLICT  // (tools/ubench experiment, wrong results: the gather without its bank conflicts)
          for (int j = 0; j < NPL; ++j) ev[i][j] = eb[i * CS + l * NPL + j];
#else
          for (int j = 0; j < NPL; ++j) ev[i][j] = eb[i * CS + g.lab[j]];
#endif
        }
        {
          // alpha[t0 + i] of the two nodes below this wave, in the previous wave's frame: 2 K consecutive floats, read in
          // 16-byte pieces (band_backward_body.inc)
          const float* bp = bnd_prev + (beta & 3) * K * 2;
          if constexpr (K % 2 == 0) {
#pragma unroll
            for (int i = 0; i < K; i += 2) {
              const gtnx_f4 q4 = *reinterpret_cast<const gtnx_f4*>(bp + 2 * i);
              bv1[i] = q4.x, bv2[i] = q4.y, bv1[i + 1] = q4.z, bv2[i + 1] = q4.w;
            }
          } else {
#pragma unroll
            for (int i = 0; i < K; ++i) bv1[i] = bp[2 * i], bv2[i] = bp[2 * i + 1];
          }
        }
#pragma unroll
        for (int q = 0; q <= NP; ++q) offp[q] = off_prev[(beta * NP + q) & 15];
        float hist[K][NPL];
#pragma unroll
        for (int i = 0; i < K; ++i) {
          if (FULL || i < rows) {
            if (i % RNk == 0) {
              // the conversion to this wave's frame is one number per shift period: added to the period's boundary
              // values two per instruction (v_pk_add_f32), not 2 RNk single adds
              typedef float f2v __attribute__((ext_vector_type(2)));
              const float dconv = float(offp[i / RNk] - off);
              const f2v d2 = {dconv, dconv};
#pragma unroll
              for (int r = i; r < i + RNk && r < K; ++r) {
                const f2v c = f2v{bv1[r], bv2[r]} + d2;
                bv1[r] = c.x, bv2[r] = c.y;
              }
            }
            const float b1 = bv1[i], b2 = bv2[i];
            const float p1 = wave_shr1(a[NPL - 1], b1);
            const float p2 = NPL == 2 ? wave_shr1(a[0], b2) : wave_shr1(p1, b2);
            float nw[NPL];
#pragma unroll
            for (int j = 0; j < NPL; ++j) {
              const float s1 = j == 0 ? p1 : a[0];
              const float s2 = j == 0 ? p2 : p1;
              float x0, x1, x2;
              if (UNIT) {  // self-loop and previous-node arc everywhere, weight 0
                x0 = a[j];
                x1 = s1;
                x2 = s2 + g.wi[2][j];
              } else {
                x0 = a[j] + g.wi[0][j];
                x1 = s1 + g.wi[1][j];
                x2 = s2 + g.wi[2][j];
              }
              nw[j] = lse3(x0, x1, x2) + ev[i][j];
            }
            if ((i + 1) % RNk == 0) {  // shift this wave's row t0 + i + 1 by its maximum
              const float mx = wave_max_of(nw, NPL);
              if (mx > DEADF) {
#pragma unroll
                for (int j = 0; j < NPL; ++j) nw[j] -= mx;
                off += double(mx);
              } else if (w > 0) {
                off = offp[(i + 1) / RNk];  // nothing alive here yet: follow the wave below
              }
              if (l == 0) {
                const int p = (t0 + i + 1) / RNk;
                off_own[p & 15] = off;
                P.aoff[1 + p * 4 + w] = off;
              }
            }
#pragma unroll
            for (int j = 0; j < NPL; ++j) hist[i][j] = a[j] = nw[j];
          }
        }
        {
          const GTNX_G char* const brow = arow;  // (uniform; the lanes that write are an exec mask around the stores only)
          arow += int64_t(NS) * 4 * rows;
#ifdef GTNX_EXP_NO_ALPHA_STORE  // (tools/ubench experiment, wrong results downstream: the sweep without its alpha rows)
          if (writer && beta < 0) {
#else
          if (writer) {  // this wave never loads from HBM, so it never waits for these
#endif
#pragma unroll
            for (int i = 0; i < K; ++i)
              if (FULL || i < rows) {
                const GTNX_G char* ri = brow + int64_t(NS) * 4 * (i + 1);
#pragma unroll
                for (int j = 0; j < NPL; ++j) *reinterpret_cast<GTNX_G float*>(const_cast<GTNX_G char*>(ri) + (aoffb + 4u * j)) = hist[i][j];
              }
          }
        }
        // boundary values of rows t0 + 1 .. t0 + rows for the wave above
        if (NPL == 1 ? l >= 62 : l == 63) {
#pragma unroll
          for (int i = 0; i < K; ++i)
            if (FULL || i < rows) {
              float* bp = bnd_own + ((((beta & 3) * K + i + 1) & (4 * K - 1))) * 2;
              if (NPL == 1) {
                bp[63 - l] = hist[i][0];
              } else {
                bp[0] = hist[i][NPL - 1];
                bp[1] = hist[i][0];
              }
            }
        }
      };
      if (beta >= 0 && beta < nblocks) {
        if (beta * K + K <= T) block(std::true_type{});
        else block(std::false_type{});
      }
      GTNX_TM(5);
      lds_barrier();
      GTNX_TM(6);
      GTNX_TM_TICK();
    }
    // score = log sum over accept nodes of alpha[T]  (shortest.cpp:153-167)
    float f = NEGF;
#pragma unroll
    for (int j = 0; j < NPL; ++j) f = fmaxf(f, g.accept[j] ? a[j] : NEGF);
    const float mx = wave_max(f);
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < NPL; ++j) s += g.accept[j] ? ex2(a[j] - mx) : 0.0f;
    s = wave_sum(s);
    if (l == 0) {
      M.fin[2 * w] = mx;
      M.fin[2 * w + 1] = s;
      M.find[w] = off;
    }
#ifdef GTNX_FWD_IDLE_FROM
  } else if (wv >= GTNX_FWD_IDLE_FROM) {
    // ------------------------------------------------------------------ waves without a role in this sweep (a workgroup
    // shared with the backward sweep's twelve, ctc_step.hip): a wave that has ended no longer counts at a barrier, so
    // these stay and meet every barrier the other roles do -- the prologue's and one per tick
    lds_barrier();
    for (int tau = 0; tau < nticks; ++tau) lds_barrier();
#endif
  } else {
    // ------------------------------------------------------------------ helpers: everything else
    const int hid = threadIdx.x - BW;
    constexpr bool vec = VEC;  // host: C % 4 == 0 and 16-byte aligned emissions
    const bool want_lse = P.norm != nullptr || P.rowlse != nullptr;
    // staging of the emission ring: chunk c = rows [cK, cK + K) = block c
    Stage<8> st[D];
    auto rows_of = [&](int c) { return c < nblocks ? min(K, T - c * K) : 0; };
    auto issue = [&](Stage<8>& s, int c) { s.template issue<VEC>(P.em + int64_t(c) * K * C, rows_of(c) * C, hid); };
    GTNX_G float* const em_copy = P.em_copy;  // (uniform; null on every path but a region's first sweep)
    // COPY is a compile-time choice (the helper's loop is instantiated twice, selected once, below): the copy's stores
    // and their address arithmetic are not in the loop of the launches that make no copy
    auto land = [&](const Stage<8>& s, int c, int c5 /* c % NBE */, auto copy_tag) {
      constexpr bool COPY = decltype(copy_tag)::value;
      float* base = ering + c5 * K * CS;
      GTNX_G float* cdst = em_copy + int64_t(c) * K * C;
      s.template each<VEC>(rows_of(c) * C, C, hid, [&](int, int e, int r, int col, gtnx_f4 q) {
        float* d = base + r * CS + col;
        if (vec) *reinterpret_cast<gtnx_f4*>(d) = gtnx_f4{em2(q.x), em2(q.y), em2(q.z), em2(q.w)};
        else d[0] = em2(q.x);
        if (COPY) {  // the values as they came (natural log), where the backward sweep will read them
          // (non-temporal: 16 bytes per lane that nothing in this launch reads again -- 0.334 -> 0.303 ms at C3; the
          //  same on the alpha rows and the gradient rows, 4 bytes per lane, measured slower and is not done)
          if (vec) __builtin_nontemporal_store(q, reinterpret_cast<GTNX_G gtnx_f4*>(cdst + e));
          else __builtin_nontemporal_store(q.x, cdst + e);
        }
      });
    };
    // row-wise log2-sum-exp2 of a landed chunk (normaliser): 256 / K lanes per row, pairs
    // (max, sum) per 16-lane group in phase A, merged per row by one lane in phase B (a tick later)
    constexpr int LPR = BW / K, G16 = LPR / 16;
    const int EPL = (C + LPR - 1) / LPR;  // <= 16
    double normacc = 0.0;
    // (N = 4 / 8 / 16 elements per lane, chosen once per launch shape: a loop over 16 with a runtime bound costs
    //  sixteen v_exp_f32 whatever the bound is -- at C = 256 half of the normaliser's transcendentals were wasted)
    auto lse_a_n = [&](int c, int c5 /* c % NBE */, auto nconst) {
      constexpr int NE = decltype(nconst)::value;
      const int rows = rows_of(c), rr = hid / LPR, sub = hid - rr * LPR;
      if (rows <= 0) return;
      const float* e = ering + (c5 * K + min(rr, rows - 1)) * CS + sub * EPL;
      float x[NE];
      float m = NEGF;
      if (VEC && (EPL & 3) == 0) {  // uniform: whole 16-byte reads (a lane's EPL values are contiguous and 16-byte aligned;
                                    // one ds_read_b128 per four values where eight 4-byte reads at a stride of EPL banks
                                    // were the forward sweep's LDS bank conflicts, profiles/r05_v2_c3_pmc_sq.json)
#pragma unroll
        for (int i = 0; i < NE; i += 4) {
          const bool in = i < EPL && sub * EPL + i < C;
          const gtnx_f4 q = in ? *reinterpret_cast<const gtnx_f4*>(e + i) : gtnx_f4{NEGF, NEGF, NEGF, NEGF};
          x[i] = q.x, x[i + 1] = q.y, x[i + 2] = q.z, x[i + 3] = q.w;
          m = fmaxf(fmaxf(m, fmaxf(q.x, q.y)), fmaxf(q.z, q.w));
        }
      } else {
#pragma unroll
        for (int i = 0; i < NE; ++i) {
          x[i] = (i < EPL && sub * EPL + i < C) ? e[i] : NEGF;
          m = fmaxf(m, x[i]);
        }
      }
      m = row16_max(m);
      float sum = 0.0f;
#pragma unroll
      for (int i = 0; i < NE; ++i) sum += (i < EPL) ? ex2(x[i] - m) : 0.0f;
      sum = row16_sum(sum);
      if ((hid & 15) == 0 && rr < rows) {
        float* p = M.lsep + (c & 1) * 256 + (rr * 8 + (sub >> 4)) * 2;
        p[0] = m;
        p[1] = sum;
      }
    };
    auto lse_a = [&](int c, int c5) {
      if (EPL <= 4) lse_a_n(c, c5, std::integral_constant<int, 4>{});        // uniform
      else if (EPL <= 8) lse_a_n(c, c5, std::integral_constant<int, 8>{});
      else lse_a_n(c, c5, std::integral_constant<int, 16>{});
    };
    auto lse_b = [&](int c) {
      const int rows = rows_of(c);
      if (hid < rows) {
        const float* p = M.lsep + (c & 1) * 256 + hid * 16;
        float Mx = p[0];
#pragma unroll
        for (int k = 1; k < G16; ++k) Mx = fmaxf(Mx, p[2 * k]);
        float S = 0.0f;
#pragma unroll
        for (int k = 0; k < G16; ++k) S += p[2 * k + 1] * ex2(p[2 * k] - Mx);
        const float l2 = Mx + lg2(S);
        if (P.rowlse) P.rowlse[c * K + hid] = l2;
        normacc += double(l2);
      }
    };
    auto run = [&](auto copy_tag) {
      // prologue: chunk 0 landed, chunks 1 .. D requested
      issue(st[0], 0);
      land(st[0], 0, 0, copy_tag);
#pragma unroll
      for (int c = 1; c <= D; ++c) issue(st[c % D], c);
      lds_barrier();
      int t5 = 0;  // tau % NBE
      for (int tau0 = 0; tau0 < nticks; tau0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
          const int tau = tau0 + d;
          if (tau >= nticks) break;
          GTNX_TM(0);
          const int n5 = t5 + 1 == NBE ? 0 : t5 + 1;  // (tau + 1) % NBE
          // chunk tau + 1 lands (its ring block was last read a tick ago), chunk tau + 1 + D is requested
          land(st[(d + 1) % D], tau + 1, n5, copy_tag);
          GTNX_TM(1);
          issue(st[(d + 1) % D], tau + 1 + D);
          GTNX_TM(2);
          if (want_lse) {
            if (tau >= 1 && tau - 1 < nblocks) lse_b(tau - 1);
            if (tau < nblocks) lse_a(tau, t5);
          }
          t5 = n5;
          GTNX_TM(4);
          lds_barrier();
          GTNX_TM(6);
          GTNX_TM_TICK();
        }
      }
    };
    // The copy variant (a region's first sweep: the emissions are also stored where the backward sweep will read
    // them) with ONE more staging set than chunks in flight, and the request made BEFORE the landing: a request into
    // the registers a store has just read has to wait for that store (the only counter is vmcnt, and the compiler
    // waits for all of it) -- the store's whole round trip, every tick.  Here the registers requested into are the
    // ones landed a tick AGO, so what the wait at the top of a tick covers is a tick old.
    auto run_copy = [&]() {
      constexpr int DC = GTNX_FWD_COPY_DEPTH < 8 / K ? 8 / K : GTNX_FWD_COPY_DEPTH;  // ticks a request is in flight
      constexpr int R = DC + 1;
      Stage<8> sc[R];
      issue(sc[0], 0);
      land(sc[0], 0, 0, std::true_type{});
#pragma unroll
      for (int c = 1; c <= DC; ++c) issue(sc[c % R], c);
      lds_barrier();
      int t5 = 0;  // tau % NBE
      for (int tau0 = 0; tau0 < nticks; tau0 += R) {
#pragma unroll
        for (int d = 0; d < R; ++d) {
          const int tau = tau0 + d;
          if (tau >= nticks) break;
          GTNX_TM(0);
          const int n5 = t5 + 1 == NBE ? 0 : t5 + 1;  // (tau + 1) % NBE
          // chunk tau + 1 + DC is requested into the set chunk tau left a tick ago ((tau + 1 + DC) % R == tau % R),
          // then chunk tau + 1 lands (its ring block was last read a tick ago)
          sc[(d + 1) % R].settle_all();
          issue(sc[d % R], tau + 1 + DC);
          GTNX_TM(2);
          land(sc[(d + 1) % R], tau + 1, n5, std::true_type{});
          GTNX_TM(1);
          if (want_lse) {
            if (tau >= 1 && tau - 1 < nblocks) lse_b(tau - 1);
            if (tau < nblocks) lse_a(tau, t5);
          }
          t5 = n5;
          GTNX_TM(4);
          lds_barrier();
          GTNX_TM(6);
          GTNX_TM_TICK();
        }
      }
    };
    if (em_copy) {  // (uniform)
      if (GTNX_FWD_COPY_ROTATE) run_copy();
      else run(std::true_type{});
    } else {
      run(std::false_type{});
    }
    if (hid < 16) M.red[hid] = normacc;
  }
  GTNX_TM_DUMP();
  lds_barrier();
  if (threadIdx.x == 0) {
    double Mx = double(NEGF);
    for (int k = 0; k < 4; ++k)
      if (M.fin[2 * k] > DEADF) Mx = fmax(Mx, M.find[k] + double(M.fin[2 * k]));
    const bool dead = !(Mx > double(DEADF));
    float S = 0.0f;
    for (int k = 0; k < 4; ++k)
      if (M.fin[2 * k] > DEADF) S += M.fin[2 * k + 1] * ex2(float(M.find[k] + double(M.fin[2 * k]) - Mx));
    const double z2 = dead ? double(NEGF) : Mx + double(lg2(S));
    P.aoff[0] = z2;
    P.score[0] = dead ? -__builtin_inff() : float(z2 * LN2);
    if (P.norm) {
      double n2 = 0.0;
      for (int k = 0; k < 16; ++k) n2 += M.red[k];
      P.norm[0] = n2 < double(DEADF) ? -__builtin_inff() : float(n2 * LN2);
    }
  }
