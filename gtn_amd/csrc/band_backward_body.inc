// band_backward_body.inc -- the body of band.hip's backward sweep kernel, included once per entry point (band.hip: the pair of a
// launch comes out of the launch's table, or -- a launch of one pair -- is the kernel's own argument).  GTNX_BAND_PAIR
// names it.  Not a translation unit of its own.
  constexpr int RNk = K >= 4 ? 4 : K;
  constexpr int NP = K / RNk;
  const BandPair P = GTNX_BAND_PAIR;
  const int T = P.T, C = P.C, NS = P.NS;
  extern __shared__ float lds[];
  const BandLds L = band_lds(C, K, NSmax, true);
  float* ering = lds + L.o_ering;  // [NBGE blocks][K][CS]   emissions (kept until the block's gradient is out)
  float* aring = lds + L.o_aring;  // [NBE blocks][K][NSmax] alpha rows
  float* oring = lds + L.o_oring;  // [NBG blocks][K][NSmax] node posteriors
  int* snode = reinterpret_cast<int*>(lds + L.o_snode);  // [n_lab] nodes sorted by (label, node)
  const BandMisc M = band_misc<K>(lds, L);
  float* lser = M.lsep;            // [NBG blocks][K] row log-sum-exp (softmax term)
  const int CS = L.CS;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool sweeper = wv < 4;
  const int l = threadIdx.x & 63;
  const int nblocks = (T + K - 1) / K;
  const int nticks = nblocks + 5;  // block c: row sums at tick c + 4, gradient rows out at tick c + 5
  const GTNX_G double* ao = P.aoff;
  const double z2 = uniform(ao[0]);
  const bool dead = !(z2 > double(DEADF));
  const float ds = uniform(P.delta[0]);
  const bool want_em = P.grad_em != nullptr;
  GTNX_TM_INIT(128);
  // ---- who does what besides the recursion.  !SPLIT (the build): the sweepers sum the rows, the draining waves write
  // every gradient row -- the form of rounds 3-4.  SPLIT (-DGTNX_BWD_SPLIT=1; two workgroups per CU, K >= 2): the row
  // sums go to the DRAINING waves (wave d sums row d) and a block's gradient rows are written half by them, half by
  // the STAGING waves, which idle through more than half of every tick (tools/ubench/band_bench_tm: sweepers 2 430
  // busy cycles per tick with the sums, drainers 2 420, stagers 1 150).  Measured in round 5 and NOT the build:
  // 0.47 against 0.42 ms -- a drain pass costs ~500 cycles before its first row (label runs, row scalars, addresses,
  // LDS round trips), so two half passes are 1 250 + 1 250 where one was 2 000, and the sums take 800 cycles in a
  // wave that is not a sweeper (drainers 2 380 per tick, sweepers idle for 1 100).
  constexpr bool SPLIT = !BIG && K >= 2 && GTNX_BWD_SPLIT;
  const float dn_k = P.delta_norm ? uniform(P.delta_norm[0]) : 0.0f;
  float* const rnorm_k = lser + NBG * K;  // [NBG blocks][K] what makes a row's posteriors sum to one
  auto rows_of_k = [&](int c) { return c < nblocks ? min(K, T - c * K) : 0; };
  // Ring positions (c % NBG, c % NBE) are carried as counters by the tick loops: the compiler's division by 7 or 5 is
  // eight scalar instructions, every tick, in instruction streams that issue one instruction per ~5 cycles whatever
  // its kind (tools/ubench/ops_rate) -- a wave's scalar bookkeeping is as dear as its arithmetic.
  auto ring_start = [](int c, int M) { return ((c % M) + M) % M; };  // (once, before a loop; c may be negative)
  static_assert((NBGE & (NBGE - 1)) == 0, "the emission ring's position is a mask");
  auto ge_of = [](int c) { return int(unsigned(c) & unsigned(NBGE - 1)); };  // c % NBGE, c >= 0
  auto ring_step = [](int& v, int M) { v = v + 1 == M ? 0 : v + 1; };
  // row sums of block c, row r, by one wave (lane l owns nodes 4l .. 4l+3, + 256 for the second read; the ring holds 0
  // for nodes past N, so only whole reads past the row are masked).  Posteriors of a time step sum to one; in
  // float32 the two sweeps and the score drift apart by ~1e-4 over a thousand steps (all nodes of a row alike): the
  // row is rescaled to its exact total -- and, having the hot label's share in hand as well, the summing wave
  // stores that gradient element.
  struct RowSumRegs {
    float in[NPL];
    gtnx_f4 hot[NPL];
  };
  auto rowsum_init = [&](RowSumRegs& R) {
#pragma unroll
    for (int q = 0; q < NPL; ++q) {
      const int mb = 256 * q + 4 * l;
      R.in[q] = mb < NSmax ? 1.0f : 0.0f;
      float hm[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int m = mb + k;
        int lab = -1;
        if (m < P.N) lab = P.nodes[m].lab;
        settle(lab);
        hm[k] = (P.hot >= 0 && lab == P.hot) ? 1.0f : 0.0f;
      }
      R.hot[q] = gtnx_f4{hm[0], hm[1], hm[2], hm[3]};
    }
  };
  // Returns the row's scale (d score / its posteriors' total), or 0 when there is none (a scale is never 0: a zero
  // d score makes every gradient 0 whatever the scale).
  // STEADY: block c is a full block of an utterance that has a path (the caller knows) -- no range test, and `dead` is
  // false at compile time: every select on a wave-uniform condition is a v_cndmask_b32, which costs a SIMD 2.6 times
  // what a v_fma_f32 does (tools/ubench/valu_tput: 5.7 against 2.2 cycles with four waves issuing)
  auto rowsum_do = [&](const RowSumRegs& R, int c, int cg /* c % NBG */, int r, auto steady_tag) -> float {
    constexpr bool STEADY = decltype(steady_tag)::value;
    if (!want_em || (K < 4 && r >= K)) return 0.0f;  // (wave r sums row r: blocks of fewer rows than sweepers leave some without)
    if constexpr (!STEADY) {
      if (r >= rows_of_k(c)) return 0.0f;
    }
    const bool dead_r = STEADY ? false : dead;
    const float* ob = oring + (cg * K + r) * NSmax;
    gtnx_f4 v[NPL];
#pragma unroll
    for (int q = 0; q < NPL; ++q) v[q] = *reinterpret_cast<const gtnx_f4*>(ob + min(256 * q + 4 * l, NSmax - 4));
    const float em_hot = ering[(ge_of(c) * K + r) * CS + max(P.hot, 0)];
    const float ls_hot = lser[cg * K + r];
    float all = (v[0].x * R.in[0] + v[0].y * R.in[0]) + (v[0].z * R.in[0] + v[0].w * R.in[0]);
    float hotp = (v[0].x * R.hot[0].x + v[0].y * R.hot[0].y) + (v[0].z * R.hot[0].z + v[0].w * R.hot[0].w);
#pragma unroll
    for (int q = 1; q < NPL; ++q) {
      all += (v[q].x * R.in[q] + v[q].y * R.in[q]) + (v[q].z * R.in[q] + v[q].w * R.in[q]);
      hotp += (v[q].x * R.hot[q].x + v[q].y * R.hot[q].y) + (v[q].z * R.hot[q].z + v[q].w * R.hot[q].w);
    }
    if (dead_r) all = hotp = 0.0f;  // nothing wrote the ring
    wave_sum63x2(all, hotp);
    all = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(all), 63));  // (uniform from here on)
    const bool have = all != 0.0f && !dead_r;
    const float f = have ? ds * __builtin_amdgcn_rcpf(all) : 1.0f;
    if (l == 63 && P.hot >= 0) {
      // (no normaliser: the staging waves put +inf where the row's log-sum-exp would be, the term is dn * 2^-inf = 0)
      const float sm = dn_k * ex2(em_hot - ls_hot);
      P.grad_em[int64_t(T - 1 - c * K - r) * C + P.hot] = (dead_r ? 0.0f : hotp * f) + sm;
    }
    if (l == 0) rnorm_k[cg * K + r] = f;
    return have ? f : 0.0f;
  };
  // ROWSUM4 (K = 4, one node per sweeper lane: C3's shape): ALL FOUR rows of a block summed by ONE wave -- sixteen lanes
  // per row, sixteen nodes per lane, a reduction inside DPP rows (four steps, no broadcast steps) -- and that wave is
  // the emission-staging wave that does not land a chunk this tick.  A wave-instruction costs the SIMD the same
  // whether 64 lanes or 16 have work: four sweepers summing a row each were 4 x ~60 instructions per tick where this is
  // ~75, and the sweep is bound by the instructions its SIMDs issue (DESIGN 13.3) -- so the move pays although the
  // earlier one of the SAME per-row sums to the staging waves (round 6, RS_STAGE) did not.  The sweepers take the
  // scale they apply to G's arc posteriors from the ring the sums publish, one tick later.
#ifndef GTNX_BWD_ROWSUM4
#define GTNX_BWD_ROWSUM4 1
#endif
  constexpr bool RS4 = !BIG && !SPLIT && K == 4 && NPL == 1 && GTNX_BWD_ROWSUM4;
  struct RowSum4Regs {
    float in;         // this lane's sixteen nodes lie inside the row (the launcher makes the ring's row stride a multiple of 16)
    gtnx_f4 hot[4];   // ... and which of them carry the hot label
    int po;           // float offset of the sixteen inside a posterior-ring block (row included)
    int eo, go;       // ... of the hot emission inside an emission-ring block, of the gradient element from the block's lowest row
  };
  auto rowsum4_init = [&](RowSum4Regs& R) {
    const int r = l >> 4, nb = 16 * (l & 15);
    R.in = nb < NSmax ? 1.0f : 0.0f;
    R.po = r * NSmax + min(nb, NSmax - 16);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float hm[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int m = nb + 4 * k + e;
        int lab = -1;
        if (m < P.N) lab = P.nodes[m].lab;
        settle(lab);
        hm[e] = (P.hot >= 0 && lab == P.hot) ? 1.0f : 0.0f;  // (nodes past the row: past N as well)
      }
      R.hot[k] = gtnx_f4{hm[0], hm[1], hm[2], hm[3]};
    }
    R.eo = r * CS + max(P.hot, 0);
    R.go = (K - 1 - r) * C + max(P.hot, 0);  // (from the block's LOWEST row: an unsigned offset beside a uniform base)
  };
  auto rowsum4_do = [&](const RowSum4Regs& R, int c, int cg /* c % NBG */, auto steady_tag) {
    constexpr bool STEADY = decltype(steady_tag)::value;  // a full block of an utterance that has a path
    const int rows = STEADY ? K : rows_of_k(c);
    if (!want_em || rows <= 0) return;
    const bool dead_r = STEADY ? false : dead;
    typedef float f2v __attribute__((ext_vector_type(2)));
    const float* ob = oring + cg * K * NSmax + R.po;
    gtnx_f4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = *reinterpret_cast<const gtnx_f4*>(ob + 4 * k);
    const float em_hot = ering[ge_of(c) * K * CS + R.eo];
    const float ls_hot = lser[cg * K + (l >> 4)];
    // (two values per instruction: the halves of a 16-byte read are register pairs as they land)
    f2v a2 = f2v{v[0].x, v[0].y} + f2v{v[0].z, v[0].w};
    f2v h2 = f2v{v[0].x, v[0].y} * f2v{R.hot[0].x, R.hot[0].y};
    h2 = __builtin_elementwise_fma(f2v{v[0].z, v[0].w}, f2v{R.hot[0].z, R.hot[0].w}, h2);
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      a2 += f2v{v[k].x, v[k].y} + f2v{v[k].z, v[k].w};
      h2 = __builtin_elementwise_fma(f2v{v[k].x, v[k].y}, f2v{R.hot[k].x, R.hot[k].y}, h2);
      h2 = __builtin_elementwise_fma(f2v{v[k].z, v[k].w}, f2v{R.hot[k].z, R.hot[k].w}, h2);
    }
#ifdef GTNX_BWD_RS4_LEAN
    // (set by a kernel that has one vector register less for this sweep -- ctc_step.hip: "is this lane's group of sixteen
    //  nodes inside the row" is worked out again at every use, a handful of instructions in a wave that idles through
    //  half of a tick, instead of living in a register across the loop; settle() keeps it from being hoisted back out)
    int nb_l = 16 * (l & 15);
    settle(nb_l);
    const float r_in = nb_l < NSmax ? 1.0f : 0.0f;
#else
    const float r_in = R.in;
#endif
    float all = (a2.x + a2.y) * r_in, hotp = h2.x + h2.y;
    if (dead_r) all = hotp = 0.0f;  // nothing wrote the ring
    row_sum15x2(all, hotp);          // totals of row r in lane 16 r + 15
    const bool have = all != 0.0f && !dead_r;
    const float f = have ? ds * __builtin_amdgcn_rcpf(all) : 1.0f;
    if ((l & 15) == 15 && (STEADY || (l >> 4) < rows)) {
      if (P.hot >= 0) {
        const float sm = dn_k * ex2(em_hot - ls_hot);  // (no normaliser: ls is +inf, the term 0)
        const GTNX_G char* gb = reinterpret_cast<const GTNX_G char*>(P.grad_em + int64_t(T - c * K - K) * C);
        *reinterpret_cast<GTNX_G float*>(const_cast<GTNX_G char*>(gb) + unsigned(4 * R.go)) = (dead_r ? 0.0f : hotp * f) + sm;
      }
      rnorm_k[cg * K + (l >> 4)] = f;
    }
  };
  // gradient rows [R0, R1) of block c (every sweeper is through with it, its rows are summed): lane `hid` of a
  // 256-lane role GATHERS the posteriors of the nodes that carry label hid (+ 256 ...), adds the normaliser's
  // softmax term and stores the finished element -- coalesced, once.  The label runs come out of the table the
  // drainers build in the posterior ring before the first tick.
  constexpr int NCS = 8 / K;  // C <= 2048 / K labels, 256 per round
  struct DrainRegs {
    int s[NCS], e[NCS], n0[NCS], n1[NCS];
    float m0[NCS], m1[NCS];
    bool more_any;
  };
  auto drain_init = [&](DrainRegs& D, int hid) {
    const int* cls = reinterpret_cast<const int*>(oring);
#pragma unroll
    for (int q = 0; q < NCS; ++q) {
      const int cc = hid + q * BW;
      D.s[q] = D.e[q] = 0;
      if (cc < C && cc != P.hot) {
        D.s[q] = cls[cc];
        D.e[q] = cls[C + cc];
      }
      const int cnt = D.e[q] - D.s[q];
      D.n0[q] = cnt > 0 ? snode[D.s[q]] : 0;
      D.n1[q] = cnt > 1 ? snode[D.s[q] + 1] : 0;
      D.m0[q] = cnt > 0 ? 1.0f : 0.0f;
      D.m1[q] = cnt > 1 ? 1.0f : 0.0f;
    }
    // (does any lane of this wave carry a label that sits on more than two nodes?  Uniform, once: the loop over the
    //  rest of such a run is a divergent one, and its tests alone cost every tick of every wave)
    D.more_any = false;
#pragma unroll
    for (int q = 0; q < NCS; ++q) D.more_any = D.more_any || __builtin_amdgcn_ballot_w64(D.e[q] - D.s[q] > 2) != 0;
  };
  // FULL: a block of K rows (every block but the last): no per-row test
  // DEADU: the utterance has no path -- the rows are the normaliser's term alone, and nothing wrote the posterior ring
  auto drain_rows = [&](const DrainRegs& D, int hid, int c, int cg /* c % NBG */, auto full_tag, auto dead_tag, auto r0_tag, auto r1_tag) {
    constexpr bool FULL = decltype(full_tag)::value;
    constexpr bool DEADU = decltype(dead_tag)::value;
    constexpr int R0 = decltype(r0_tag)::value, R1 = decltype(r1_tag)::value;
    const int rows = FULL ? K : rows_of_k(c);
    const float* ob = oring + cg * K * NSmax;
    const float* eb = ering + ge_of(c) * K * CS;
    const float* lb = lser + cg * K;
    const float* fb = rnorm_k + cg * K;
    GTNX_G float* dst = P.grad_em + int64_t(T - 1 - c * K) * C;  // row r of the block is t = T-1-cK-r
#pragma unroll
    for (int q = 0; q < NCS; ++q) {
      if (q > 0 && q * BW >= C) break;  // uniform
      const int cc = hid + q * BW;
      const bool mine = cc < C && cc != P.hot;
      // every LDS read of the rows first (addresses are known up front), then the arithmetic
      float p0[K], p1[K], e[K], ls[K], f[K];
#pragma unroll
      for (int r = R0; r < R1; ++r) {
        if constexpr (!DEADU) {
          p0[r] = ob[r * NSmax + D.n0[q]];
          p1[r] = ob[r * NSmax + D.n1[q]];
        }
        e[r] = eb[r * CS + min(cc, C - 1)];
      }
      if constexpr (K == 4) {  // the rows' scalars: two 16-byte broadcast reads
        const gtnx_f4 l4 = *reinterpret_cast<const gtnx_f4*>(lb), f4 = *reinterpret_cast<const gtnx_f4*>(fb);
        ls[0] = l4.x, ls[1] = l4.y, ls[2] = l4.z, ls[3] = l4.w;
        f[0] = f4.x, f[1] = f4.y, f[2] = f4.z, f[3] = f4.w;
      } else {
#pragma unroll
        for (int r = R0; r < R1; ++r) {
          ls[r] = lb[r];
          f[r] = fb[r];
        }
      }
      float sum[K];
      if constexpr (!DEADU) {
#pragma unroll
      for (int r = R0; r < R1; ++r) sum[r] = p0[r] * D.m0[q] + p1[r] * D.m1[q];
      }
      if (!DEADU && D.more_any) {  // uniform
        for (int i = D.s[q] + 2; i < D.e[q]; ++i) {  // (a label on more than two nodes)
          const float* o = ob + snode[i];
#pragma unroll
          for (int r = R0; r < R1; ++r) sum[r] += o[r * NSmax];
        }
      }
      float val[K];
#pragma unroll
      for (int r = R0; r < R1; ++r) {
        const float sm = dn_k * ex2(e[r] - ls[r]);  // (no normaliser: ls is +inf, see rowsum_do)
        val[r] = DEADU ? sm : sum[r] * f[r] + sm;
      }
      if (mine) {  // one exec mask for the block's stores; a row's address is a uniform base + this lane's label
#pragma unroll
        for (int r = R0; r < R1; ++r) {
          if (FULL || r < rows) {
            GTNX_G float* row = dst - int64_t(r) * C;
            row[cc] = val[r];
          }
        }
      }
    }
  };
  auto drain_block = [&](const DrainRegs& D, int hid, int c, int cg, auto r0_tag, auto r1_tag) {
    if (!want_em || c >= nblocks) return;
    if (dead) drain_rows(D, hid, c, cg, std::false_type{}, std::true_type{}, r0_tag, r1_tag);
    else if (c * K + K <= T) drain_rows(D, hid, c, cg, std::true_type{}, std::false_type{}, r0_tag, r1_tag);
    else drain_rows(D, hid, c, cg, std::false_type{}, std::false_type{}, r0_tag, r1_tag);
  };
  constexpr int KH = SPLIT ? K / 2 : K;  // rows of a block the draining waves write

  if (sweeper) {
#ifndef GTNX_BWD_SWEEP_PRIO
#define GTNX_BWD_SWEEP_PRIO 1
#endif
    __builtin_amdgcn_s_setprio(GTNX_BWD_SWEEP_PRIO);  // the recursion is the critical path; the staging waves of the CU's other workgroup yield (2 %)
    // ------------------------------------------------------------------ the recursion: no global loads in the loop
    const int w = wv;
    const int lag = 3 - w;
    const int m0 = threadIdx.x * NPL;
    NodeRegs<NPL> g;
    load_nodes<NPL, true>(P, m0, g);
    float b[NPL], post[NPL], acc[3][NPL];
    // frames: true alpha[r] = stored + ao[1 + (r >> lgrn) * 4 + w] (periods of the FORWARD launch); true beta = b + bsum
    const double Ahi = uniform(ao[1 + (T >> P.lgrn) * 4 + w]);
    double bsum = 0.0;
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
      b[j] = g.accept[j] ? 0.0f : NEGF;
      float ahi = m0 < NS ? P.alpha[int64_t(T) * NS + m0 + j] : NEGF;
      settle(ahi);
      // posterior of node n at time T (gradient row T-1); every later one comes out of the recursion
      post[j] = dead ? 0.0f : ex2(ahi + b[j] + float(Ahi - z2));  // (the row scale carries d score)
      acc[0][j] = acc[1][j] = acc[2][j] = 0.0f;
      settle(g.lab[j]);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        settle(g.wo[k][j]);
        settle(g.ao[k][j]);
      }
    }
    // pipeline position s = 3 - w: this wave publishes into region s + 1 and reads region s (0: constants)
    float* bnd_own = M.bndr + (4 - w) * 4 * K * 2;
    const float* bnd_prev = M.bndr + (3 - w) * 4 * K * 2;
    double* off_own = M.offr + (4 - w) * 16;
    const double* off_prev = M.offr + (3 - w) * 16;
    if (threadIdx.x < 8 * K) M.bndr[threadIdx.x] = NEGF;
    if (threadIdx.x < 16) M.offr[threadIdx.x] = 0.0;
    if (l == 0) off_own[0] = 0.0;
    lds_barrier();  // (the helpers sort labels in the posterior ring ...
    lds_barrier();  //  ... done)
    RowSumRegs rsr;
    if constexpr (!SPLIT && !RS4) rowsum_init(rsr);
    // G's arc gradients are sums over T of arc posteriors, and a time step's arc posteriors carry the same common
    // drift as its node posteriors (~1e-4 over a thousand steps, see rowsum_do; measured 3.9e-4 on the summed arc
    // gradients at T = 1000, tests/test_batch_gpu.py).  The exact scale of a row is known four ticks after the row;
    // the drift is smooth and zero where the sweep starts (beta is exact at T), so a block's arc posteriors are
    // scaled with the newest row scale this wave has summed -- 1 to 4 blocks old -- as they join the accumulators.
    float gscale = ds;
    // beta % NBE, beta % NBG, (tau - 4) % NBG (ROWSUM4: (tau - 5) % NBG, the block whose scales were published a tick ago)
    int bm5 = ring_start(-lag, NBE), bm7 = ring_start(-lag, NBG), rm7 = ring_start(RS4 ? -5 : -4, NBG);
    lds_barrier();  // the label table is in registers: the posterior ring may be written
    // A tick as a function of (tau, STEADY).  STEADY: this wave has a FULL block to sweep and a full block to sum -- every
    // tick but the first four and the last few -- and none of the tick's range tests is compiled in (they were ~20
    // scalar instructions per tick in a stream of ~340).
    auto tick = [&](int tau, auto steady_tag) {
      constexpr bool STEADY = decltype(steady_tag)::value;
      GTNX_TM(0);
      // (the last wave left block tau - 4 a tick ago.  SPLIT: the draining waves take the sums, see the head of the kernel)
      if constexpr (RS4) {
#ifndef GTNX_EXP_NO_GSCALE
        // Row w of block tau - 5, published a tick ago.  Read whenever that block is a full one (every block this wave
        // still has rows to sweep after is), no test of the value: a row without posterior mass publishes 1, and the arc
        // posteriors it would scale are as absent as the mass.
        if (GRADG && want_em && (STEADY || (tau >= 5 && (tau - 5) * K + K <= T))) gscale = rnorm_k[rm7 * K + w];
#endif
      } else if constexpr (!SPLIT) {
#ifndef GTNX_EXP_NO_ROWSUM
        if (STEADY || tau >= 4) {
          const float fr = rowsum_do(rsr, tau - 4, rm7, w, steady_tag);
#ifndef GTNX_EXP_NO_GSCALE
          if (fr != 0.0f) gscale = fr;  // (uniform)
#endif
        }
#endif
      }
      GTNX_TM(3);
      const int beta = tau - lag;
      // (full blocks are compiled without the per-row tests, as in the forward sweep)
      auto block = [&](auto full_tag) {
        constexpr bool FULL = decltype(full_tag)::value;
        const int v0 = beta * K, rows = FULL ? K : min(K, T - v0);
        const float* eb = ering + ge_of(beta) * K * CS;
        const float* ab = aring + bm5 * K * NSmax;
        const double* Ab = M.aofr + (bm5 * K) * 4 + w;
        float* ob = oring + bm7 * K * NSmax + m0;
        float ev[K][NPL], alov[K][NPL], bq1[K], bq2[K];
        double Acur[K], offp[NP + 1];
#pragma unroll
        for (int i = 0; i < K; ++i) {
#pragma unroll
          for (int j = 0; j < NPL; ++j) {
            ev[i][j] = eb[i * CS + g.lab[j]];
            alov[i][j] = ab[i * NSmax + min(m0 + j, NS - 1)];  // (landed data only: lanes past N stay finite)
          }
          Acur[i] = Ab[i * 4];
        }
#pragma unroll
        for (int q = 0; q <= NP; ++q) offp[q] = off_prev[(beta * NP + q) & 15];
        {
          // q[v0 + i] of the two nodes above this wave, in the next wave's frame: the block's K pairs are 2 K consecutive
          // floats, 32-byte aligned -- read in 16-byte pieces (a ds_read2_b32 per row came with a scalar add and a
          // v_mov each for its address).  NP == 1 (every backward shape): the conversion to this wave's frame is one
          // number per block, known here -- added two values per instruction (v_pk_add_f32) instead of 2 K single adds
          const float* bp = bnd_prev + (beta & 3) * K * 2;
          if constexpr (K % 2 == 0) {
            typedef float f2v __attribute__((ext_vector_type(2)));
            const float dc0 = NP == 1 ? float(offp[0] - bsum) : 0.0f;
            const f2v dc2 = {dc0, dc0};
#pragma unroll
            for (int i = 0; i < K; i += 2) {
              const gtnx_f4 q4 = *reinterpret_cast<const gtnx_f4*>(bp + 2 * i);
              const f2v a = f2v{q4.x, q4.y} + dc2, b2 = f2v{q4.z, q4.w} + dc2;
              bq1[i] = a.x, bq2[i] = a.y, bq1[i + 1] = b2.x, bq2[i + 1] = b2.y;
            }
          } else {
#pragma unroll
            for (int i = 0; i < K; ++i) bq1[i] = bp[2 * i], bq2[i] = bp[2 * i + 1];
          }
        }
        constexpr bool PRECONV = NP == 1 && K % 2 == 0;  // bq1 / bq2 are in this wave's frame already
        float qh[K][NPL];
        float dconv = 0.0f;
        float postv[K][NPL];
        float accb[3][NPL];  // this block's arc posteriors
#pragma unroll
        for (int j = 0; j < NPL; ++j) accb[0][j] = accb[1][j] = accb[2][j] = 0.0f;
#pragma unroll
        for (int i = 0; i < K; ++i) {
          if (FULL || i < rows) {
            if (!PRECONV && i % RNk == 0) dconv = float(offp[i / RNk] - bsum);
            float q[NPL];
#pragma unroll
            for (int j = 0; j < NPL; ++j) qh[i][j] = q[j] = ev[i][j] + b[j];
            // node posteriors at time t+1 (they belong to gradient row t): carried over from the step before; stored
            // after the block's last step, all K rows under ONE exec mask (a masked store per row was two scalar
            // instructions per row in front of the recursion)
#pragma unroll
            for (int j = 0; j < NPL; ++j) postv[i][j] = post[j];
            const float f1 = PRECONV ? bq1[i] : bq1[i] + dconv, f2 = PRECONV ? bq2[i] : bq2[i] + dconv;
            const float n1 = wave_shl1(q[0], f1);
            const float n2 = NPL == 2 ? wave_shl1(q[NPL - 1], f2) : wave_shl1(n1, f2);
            const float dl = float(Acur[i] + (bsum - z2));
            float nb[NPL];
#pragma unroll
            for (int j = 0; j < NPL; ++j) {
              const float s1 = j + 1 < NPL ? q[NPL - 1] : n1;
              const float s2 = j + 1 < NPL ? n1 : n2;
              float y0, y1, y2;
              if (UNIT) {
                y0 = q[j];
                y1 = s1;
                y2 = s2 + g.wo[2][j];
              } else {
                y0 = q[j] + g.wo[0][j];
                y1 = s1 + g.wo[1][j];
                y2 = s2 + g.wo[2][j];
              }
              // 2^(alpha[t][n] + y_k - score) is the posterior of arc k leaving (t, n); their sum S is the posterior of
              // node n at time t -- the NEXT row's gradient term -- and beta[t][n] = log2(S) - (alpha[t][n] - score): three
              // exponentials, one logarithm and ten additions per node and step.  (Rounds 3-6 shifted the three terms by
              // their maximum first and multiplied by 2^(alpha + max - score) afterwards: one exponential, one maximum and
              // three multiplies more.  No shift is needed: an arc's posterior is at most 1.  One below 2^-126 is flushed
              // to zero and beta of a node ALL of whose arcs are becomes -inf: every path through it carries less than
              // 2^-124 of the total mass, which is what the gradients lose -- DESIGN 13.3.)
#ifndef GTNX_BWD_SHIFTED
              const float cj = alov[i][j] + dl;
              const float p0 = ex2(y0 + cj), p1 = ex2(y1 + cj), p2 = ex2(y2 + cj);
              const float S = (p0 + p1) + p2;
              if (GRADG) {
                accb[0][j] += p0;
                accb[1][j] += p1;
                accb[2][j] += p2;
              }
              nb[j] = lg2(S) - cj;
              post[j] = S;
#else
              const float mx = fmaxf(fmaxf(y0, y1), y2);
              const float f = ex2(alov[i][j] + mx + dl);
              float S;
              if (GRADG) {
                const float e0 = ex2(y0 - mx), e1 = ex2(y1 - mx), e2 = ex2(y2 - mx);
                S = e0 + e1 + e2;
                accb[0][j] += e0 * f;
                accb[1][j] += e1 * f;
                accb[2][j] += e2 * f;
              } else {  // the largest term is exactly 1
                const float md = __builtin_amdgcn_fmed3f(y0, y1, y2), mn = fminf(fminf(y0, y1), y2);
                S = 1.0f + ex2(md - mx) + ex2(mn - mx);
              }
              nb[j] = mx + lg2(S);
              post[j] = f * S;
#endif
            }
            if ((i + 1) % RNk == 0) {  // shift this wave's beta row v0 + i + 1 by its maximum
              const float mx = wave_max_of(nb, NPL);
              if (mx > DEADF) {  // (uniform)
#pragma unroll
                for (int j = 0; j < NPL; ++j) nb[j] -= mx;
                bsum += double(mx);
              } else {
                // (a wave none of whose nodes is alive yet -- the band's corners.  Kept a BRANCH: as selects the two cases
                //  were four v_cndmask_b32 on the halves of two doubles in every block of every wave)
                asm volatile("; no live node in this wave's row");
                if (w < 3) bsum = offp[(i + 1) / RNk];
              }
              if (l == 0) off_own[((v0 + i + 1) / RNk) & 15] = bsum;
            }
#pragma unroll
            for (int j = 0; j < NPL; ++j) b[j] = nb[j];
          }
        }
        if (want_em && m0 < NSmax) {
#pragma unroll
          for (int i = 0; i < K; ++i)
            if (FULL || i < rows) {
#pragma unroll
              for (int j = 0; j < NPL; ++j) ob[i * NSmax + j] = postv[i][j];
            }
        }
        if (GRADG) {
#pragma unroll
          for (int j = 0; j < NPL; ++j)
#pragma unroll
            for (int k = 0; k < 3; ++k) acc[k][j] += accb[k][j] * gscale;
        }
        // q of this wave's first two nodes for the wave below
        if (NPL == 1 ? l < 2 : l == 0) {
#pragma unroll
          for (int i = 0; i < K; ++i)
            if (FULL || i < rows) {
              float* bp = bnd_own + ((beta & 3) * K + i) * 2;
              if (NPL == 1) {
                bp[l] = qh[i][0];
              } else {
                bp[0] = qh[i][0];
                bp[1] = qh[i][NPL - 1];
              }
            }
        }
      };
      if constexpr (STEADY) {
        block(std::true_type{});
      } else if (beta >= 0 && beta < nblocks && !dead) {
        if (beta * K + K <= T) block(std::true_type{});
        else block(std::false_type{});
      }
      GTNX_TM(5);
      lds_barrier();
      GTNX_TM(6);
      GTNX_TM_TICK();
    };
    {
      // steady ticks: tau >= 4 (a block to sum) and 0 <= beta < T / K (a full block to sweep); beta = tau - lag, lag <= 3
      const int s0 = min(RS4 ? 5 : 4, nticks), s1 = dead ? s0 : max(s0, min(nticks, T / K + lag));
      auto step_rings = [&]() { ring_step(bm5, NBE), ring_step(bm7, NBG), ring_step(rm7, NBG); };
      int tau = 0;
      for (; tau < s0; ++tau, step_rings()) tick(tau, std::false_type{});
      for (; tau < s1; ++tau, step_rings()) tick(tau, std::true_type{});
      for (; tau < nticks; ++tau, step_rings()) tick(tau, std::false_type{});
    }
    GTNX_TM_DUMP();
    // (EVERY arc of G is the out-arc of one node of some sweeper lane, so this writes the whole array -- zeros when no
    //  path exists: the host does not zero-fill it for targets whose arcs all lie in the band, batch.cpp BFsBandOp)
    if (GRADG && P.grad_fixed) {
#pragma unroll
      for (int j = 0; j < NPL; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k)
          if (g.ao[k][j] >= 0) P.grad_fixed[g.ao[k][j]] = dead ? 0.0f : acc[k][j];  // (scaled as they were summed: gscale carries d score)
    }
  } else if (wv < 8) {
    // ------------------------------------------------------------------ stagers (waves 4-7): emissions and alpha rows into LDS
    const bool soft = P.delta_norm != nullptr && P.rowlse != nullptr;
    lds_barrier();  // (the drainers clear the label table ...
    if constexpr (!BIG) {
      // One stream per wave: waves 4, 5 stage the emissions of the even / odd chunks, waves 6, 7 the alpha rows and
      // the rows' scalars.  (Both streams in every staging wave -- 2 x 20 staging registers -- made the kernel need
      // 96 registers where six waves per SIMD, i.e. two workgroups of twelve waves per CU, leave 80.)  A wave lands
      // chunk c and requests chunk c + 2 of its stream: a load has two ticks to arrive.
      // chunk c = virtual rows [cK, cK + rows), i.e. t from T-1-cK down; chunk row r (HBM order, ascending t) is row
      // rows-1-r of its ring block; emissions land during tick c-2 (their ring has a block to spare), alpha rows
      // and scalars during tick c-1
      const int h = wv - 4, q = h & 1;
      auto rows_of = [&](int c) { return c < nblocks ? min(K, T - c * K) : 0; };
      auto tlo_of = [&](int c) { return T - c * K - rows_of(c); };
      // SPLIT: the upper half of every block's gradient rows is written here (lane hid_s of the four staging waves
      // = label hid_s), after the tick's landing and requests
      DrainRegs dr_s;
      const int hid_s = threadIdx.x - BW;
      auto drain_upper = [&](int tau) {
        if constexpr (SPLIT) {
          if (tau >= 5) drain_block(dr_s, hid_s, tau - 5, (tau - 5) % NBG, std::integral_constant<int, KH>{}, std::integral_constant<int, K>{});
        }
      };
      if (h < 2) {
        Stage<16, 64> se;
        if constexpr (VEC) se.init_offsets(C, CS, K, l);
        // (steady_tag: the chunk is a full block of K rows -- every tick but the first and the last few; its size, its
        //  lane masks and its clamped offsets are then the same every tick and leave the loop)
        auto issue_em = [&](int c, auto steady_tag) {
          constexpr bool ST = decltype(steady_tag)::value;
          const int rows = ST ? K : rows_of(c);
          se.template issue<VEC>(P.em + int64_t(T - c * K - rows) * C, rows * C, l);
        };
        auto land_em = [&](int c, auto steady_tag) {
          constexpr bool ST = decltype(steady_tag)::value;
          const int rows = ST ? K : rows_of(c);
          se.settle_all();
          GTNX_TM(4);
          if (rows <= 0) return;
          float* eb = ering + ge_of(c) * K * CS;
          if constexpr (VEC) {
            se.each_vec(rows * C, (K - rows) * CS, l, [&](int, int o, gtnx_f4 v4) {
              typedef float f2v __attribute__((ext_vector_type(2)));  // em2 of four values: two packed multiplies
              const f2v lo = f2v{v4.x, v4.y} * LOG2E, hi = f2v{v4.z, v4.w} * LOG2E;
              *reinterpret_cast<gtnx_f4*>(eb + o) = gtnx_f4{fmaxf(lo.x, NEGF), fmaxf(lo.y, NEGF), fmaxf(hi.x, NEGF), fmaxf(hi.y, NEGF)};
            });
          } else {
            se.template each<false>(rows * C, C, l, [&](int, int, int r, int col, gtnx_f4 v4) {
              eb[(rows - 1 - r) * CS + col] = em2(v4.x);
            });
          }
        };
        issue_em(q, std::false_type{});  // prologue: the emissions of chunks 0 and 1 landed, 2 and 3 requested
        land_em(q, std::false_type{});
        issue_em(q + 2, std::false_type{});
        RowSum4Regs rs4;
        if constexpr (RS4) rowsum4_init(rs4);
        lds_barrier();
        if constexpr (SPLIT) drain_init(dr_s, hid_s);  // (the table is complete; the sweepers overwrite it after the next barrier)
        lds_barrier();  // (... and have taken their label runs)
        int r7 = ring_start(-4, NBG);  // (tau - 4) % NBG
        auto tick = [&](int tau, auto steady_tag) {
          constexpr bool ST = decltype(steady_tag)::value;
          GTNX_TM(0);
#ifndef GTNX_EXP_NO_STAGE
          if (((tau + 2) & 1) == q) {  // uniform
            land_em(tau + 2, steady_tag);
            GTNX_TM(1);
            issue_em(tau + 4, steady_tag);
            GTNX_TM(2);
          } else if constexpr (RS4) {
            // (the last sweeper left block tau - 4 a tick ago; its rows are drained a tick from now)
#ifndef GTNX_EXP_NO_ROWSUM
            if (ST || tau >= 4) rowsum4_do(rs4, tau - 4, r7, steady_tag);
#endif
          }
#endif
          drain_upper(tau);
          GTNX_TM(3);
          lds_barrier();
          GTNX_TM(6);
          GTNX_TM_TICK();
        };
        {
          // steady: chunks tau + 2 and tau + 4 and block tau - 4 are full blocks, the utterance has a path
          const int s0 = min(4, nticks), s1 = dead ? s0 : max(s0, min(nticks, T / K - 4));
          int tau = 0;
          for (; tau < s0; ++tau, ring_step(r7, NBG)) tick(tau, std::false_type{});
          for (; tau < s1; ++tau, ring_step(r7, NBG)) tick(tau, std::true_type{});
          for (; tau < nticks; ++tau, ring_step(r7, NBG)) tick(tau, std::false_type{});
        }
      } else {
        Stage<16, 64> sa;
        sa.init_offsets(NS, NSmax, K, l);
        float lse_s = __builtin_inff();  // (no normaliser: its term of a gradient element is dn * 2^(e - inf) = 0, no select)
        double af_s = 0.0;
        auto issue_rest = [&](int c, auto steady_tag) {
          constexpr bool ST = decltype(steady_tag)::value;
          const int rows = ST ? K : rows_of(c), tlo = T - c * K - rows;
          sa.template issue<true>(P.alpha + int64_t(tlo) * NS, rows * NS, l);
          if (rows > 0) {  // uniform; unconditional clamped loads (see Stage::issue)
            if (soft) lse_s = P.rowlse[tlo + min(l, rows - 1)];
            // alpha frame of ring row i = l / 4 (t = T-1-cK-i) for sweeper wave l % 4
            af_s = ao[1 + ((T - 1 - c * K - min(l >> 2, rows - 1)) >> P.lgrn) * 4 + (l & 3)];
          }
        };
        auto land_rest = [&](int c, int c5 /* c % NBE */, int c7 /* c % NBG */, auto steady_tag) {
          constexpr bool ST = decltype(steady_tag)::value;
          const int rows = ST ? K : rows_of(c);
          sa.settle_all();
          asm volatile("" : "+v"(lse_s), "+v"(af_s));
          if (rows <= 0) return;
          float* ab = aring + c5 * K * NSmax;
          sa.each_vec(rows * NS, (K - rows) * NSmax, l, [&](int, int o, gtnx_f4 v4) { *reinterpret_cast<gtnx_f4*>(ab + o) = v4; });
          if (l < rows) lser[c7 * K + rows - 1 - l] = lse_s;
          if (l < 4 * rows) M.aofr[(c5 * K) * 4 + l] = af_s;
        };
        issue_rest(q, std::false_type{});  // prologue: chunk 0 landed, chunk 1 (lands in tick 0) and chunk 2 requested
        if (q == 0) {
          land_rest(0, 0, 0, std::false_type{});
          issue_rest(2, std::false_type{});
        }
        lds_barrier();
        if constexpr (SPLIT) drain_init(dr_s, hid_s);
        lds_barrier();  // (... and have taken their label runs)
        int s5 = ring_start(1, NBE), s7 = ring_start(1, NBG);  // (tau + 1) % NBE, % NBG
        auto tick = [&](int tau, auto steady_tag) {
          GTNX_TM(0);
#ifndef GTNX_EXP_NO_STAGE
          if (((tau + 1) & 1) == q) {  // uniform
            land_rest(tau + 1, s5, s7, steady_tag);
            GTNX_TM(1);
            issue_rest(tau + 3, steady_tag);
            GTNX_TM(2);
          }
#endif
          drain_upper(tau);
          GTNX_TM(3);
          lds_barrier();
          GTNX_TM(6);
          GTNX_TM_TICK();
        };
        {
          const int s1 = max(0, min(nticks, T / K - 3));  // steady: chunks tau + 1 and tau + 3 are full blocks
          auto step_rings = [&]() { ring_step(s5, NBE), ring_step(s7, NBG); };
          int tau = 0;
          for (; tau < s1; ++tau, step_rings()) tick(tau, std::true_type{});
          for (; tau < nticks; ++tau, step_rings()) tick(tau, std::false_type{});
        }
      }
      GTNX_TM_DUMP();
    } else {
      // BIG shapes (one workgroup per CU, registers to spare, short ticks): both streams in every staging wave,
      // four ticks for a load to arrive
    // ---- staging: chunk c = virtual rows [cK, cK + rows), i.e. t from T-1-cK down; HBM rows tlo ..
    // Helper wave h owns the chunks c = h (mod 4): it lands chunk c during tick c - 1 and then
    // requests chunk c + 4, so a load has four ticks to arrive and a wave only ever waits for its
    // OWN loads (vmcnt is per wave) -- with one wave staging every chunk the compiler's counter
    // made each request wait for the chunk requested a tick earlier.
    const int h = wv - 4;
    Stage<BIG ? 32 : 16, 64> se, sa;  // K C and K NS floats over 64 lanes (<= 1024, BIG: <= 2048)
    if constexpr (VEC) se.init_offsets(C, CS, K, l);
    sa.init_offsets(NS, NSmax, K, l);
    float lse_s = __builtin_inff();
    double af_s = 0.0;
    auto rows_of = [&](int c) { return c < nblocks ? min(K, T - c * K) : 0; };
    auto tlo_of = [&](int c) { return T - c * K - rows_of(c); };
    auto issue = [&](int c) {
      const int rows = rows_of(c), tlo = tlo_of(c);
      se.template issue<VEC>(P.em + int64_t(tlo) * C, rows * C, l);
      sa.template issue<true>(P.alpha + int64_t(tlo) * NS, rows * NS, l);
      if (rows > 0) {  // uniform; unconditional clamped loads (see Stage::issue)
        if (soft) lse_s = P.rowlse[tlo + min(l, rows - 1)];
        // alpha frame of ring row i = l / 4 (t = T-1-cK-i) for sweeper wave l % 4
        af_s = ao[1 + ((T - 1 - c * K - min(l >> 2, rows - 1)) >> P.lgrn) * 4 + (l & 3)];
      }
    };
    // chunk row r (HBM order, ascending t) is row rows-1-r of its ring block.  A chunk lands in two
    // halves a tick apart -- emissions during tick c-2 (their ring has a block to spare), alpha rows and
    // the rows' scalars during tick c-1 -- so that no wave carries a whole chunk's landing in one tick:
    // the landing wave was the critical path of a tick
    auto land_em = [&](int c) {
      const int rows = rows_of(c);
      se.settle_all();
      sa.settle_all();
      asm volatile("" : "+v"(lse_s), "+v"(af_s));
      GTNX_TM(4);
      if (rows <= 0) return;
      float* eb = ering + ge_of(c) * K * CS;
      if constexpr (VEC) {
        se.each_vec(rows * C, (K - rows) * CS, l, [&](int, int o, gtnx_f4 q) {
          *reinterpret_cast<gtnx_f4*>(eb + o) = gtnx_f4{em2(q.x), em2(q.y), em2(q.z), em2(q.w)};
        });
      } else {
        se.template each<false>(rows * C, C, l, [&](int, int, int r, int col, gtnx_f4 q) {
          eb[(rows - 1 - r) * CS + col] = em2(q.x);
        });
      }
    };
    auto land_rest = [&](int c) {
      const int rows = rows_of(c);
      sa.settle_all();
      asm volatile("" : "+v"(lse_s), "+v"(af_s));
      if (rows <= 0) return;
      float* ab = aring + (c % NBE) * K * NSmax;
      sa.each_vec(rows * NS, (K - rows) * NSmax, l, [&](int, int o, gtnx_f4 q) { *reinterpret_cast<gtnx_f4*>(ab + o) = q; });
      if (l < rows) lser[(c % NBG) * K + rows - 1 - l] = lse_s;
      if (l < 4 * rows) M.aofr[((c % NBE) * K) * 4 + l] = af_s;
    };
    // prologue: chunk 0 landed, the emissions of chunk 1 too, chunks 1 .. 4 requested
    issue(h);
    if (h == 0) {
      land_em(0);
      land_rest(0);
      issue(4);
    }
    if (h == 1) land_em(1);
    lds_barrier();
    lds_barrier();  // (... and have taken their label runs)
    for (int tau = 0; tau < nticks; ++tau) {
      GTNX_TM(0);
#ifndef GTNX_EXP_NO_STAGE
      if (((tau + 1) & 3) == h) {  // uniform
        land_rest(tau + 1);
        GTNX_TM(1);
        issue(tau + 5);
        GTNX_TM(2);
      }
      if (((tau + 2) & 3) == h) {  // uniform
        land_em(tau + 2);
        GTNX_TM(1);
      }
#endif
      GTNX_TM(3);
      lds_barrier();
      GTNX_TM(6);
      GTNX_TM_TICK();
    }
    GTNX_TM_DUMP();
    }
  } else {
    // ------------------------------------------------------------------ drainers (waves 8-11): the gradient rows
    // (a role of its own since round 3: the staging wave that landed, requested AND drained in one tick was the
    //  tick's critical path, and one role per code path needs 60-odd registers where the merged helper needed 104)
    const int hid = threadIdx.x - 2 * BW;
    const bool soft = P.delta_norm != nullptr && P.rowlse != nullptr;
    // label -> run of nodes in snode (table built in the posterior ring, which is idle until the first tick)
    int* cls = reinterpret_cast<int*>(oring);
    for (int c = hid; c < 2 * C; c += BW) cls[c] = 0;
    lds_barrier();
    for (int i = hid; i < P.n_lab; i += BW) {
      const int lab = P.slab[i];
      snode[i] = P.snode[i];
      if (i == 0 || P.slab[i - 1] != lab) cls[lab] = i;
      if (i == P.n_lab - 1 || P.slab[i + 1] != lab) cls[C + lab] = i + 1;
    }
    lds_barrier();  // (the label table is complete; the stagers have landed the first chunks)
    // this lane's labels (tid, tid + 256, ...): run of nodes, the first two inline
    DrainRegs dr;
    drain_init(dr, hid);
    RowSumRegs rsr;
    if constexpr (SPLIT) rowsum_init(rsr);
    const int dw = wv - 8;  // (SPLIT: this wave sums row dw)
    lds_barrier();  // (label runs are in registers; the posterior ring is the sweepers')
    int d7 = ring_start(-5, NBG);  // (tau - 5) % NBG
    // (a steady-state split of THIS loop, as in the sweepers', measured slower: 0.414 against 0.405 ms -- the drainers are not
    //  the stream the tick waits for, and a faster drainer only takes issue slots from the sweepers earlier in the tick)
    for (int tau = 0; tau < nticks; ++tau, ring_step(d7, NBG)) {
      GTNX_TM(0);
#ifndef GTNX_EXP_NO_DRAIN  // (tools/ubench experiments: what the tick costs without the gradient rows / the staging)
      if (tau >= 5) drain_block(dr, hid, tau - 5, d7, std::integral_constant<int, 0>{}, std::integral_constant<int, KH>{});
#endif
      if constexpr (SPLIT) {  // the last sweeper left block tau - 4 a tick ago; its rows are drained a tick from now
        if (tau >= 4) rowsum_do(rsr, tau - 4, (tau - 4) % NBG, dw, std::false_type{});
      }
      GTNX_TM(3);
      lds_barrier();
      GTNX_TM(6);
      GTNX_TM_TICK();
    }
    GTNX_TM_DUMP();
  }
