// ctc_step.hip -- one CTC criterion step of a batch in ONE launch: workgroup b builds utterance b's target records,
// runs the forward band sweep (with the chain's own forwardScore fused, as band.hip does), writes
// loss_b = forwardScore(emissions_b) - forwardScore(target_b o emissions_b), and runs the backward band sweep with the
// upstream gradients -1 (score) and +1 (normaliser) -- what ctc_targets_kernel, band_forward_kernel, vec_axpby_kernel,
// scalar_seed_kernel and band_backward_kernel do in five launches (and two table uploads) through the graph-level
// operations.  Nothing in a step crosses utterances, so there is no grid-wide synchronisation: the phases of a
// workgroup are separated by a workgroup-scope release / acquire fence and a workgroup barrier, two per utterance.
//
// The sweeps are band.hip's, by inclusion of the same bodies (band_forward_body.inc, band_backward_body.inc): same
// arithmetic, same results bit for bit.  The workgroup has the backward sweep's twelve waves; in the forward phase
// waves 8-11 only keep the barrier count (GTNX_FWD_IDLE_FROM).  LDS is the larger of the two sweeps' carves, which is
// the backward sweep's at every shape this kernel is instantiated for: two workgroups per CU, as before.
//
// Cells: one node per lane (at most 256 nodes), CTC targets (unit weights), 16-byte emission rows (C % 4 == 0), not
// BIG; (rows per block forward, backward) as band_block_rows gives them: (8, 4), (8, 2), (4, 2).  ctc_step_cell()
// says whether a shape has a cell; everything else stays on the graph-level path (batch.cpp: ctc_step_fused_ok).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <stdexcept>
#include <type_traits>

#include "kernels.h"

namespace gtnx {
namespace {

#include "band_device.inc"

// the upstream gradients of a loss = norm - score whose own gradient is 1: what scalar_seed_kernel and the subtract's
// gradient function leave in the batch records' gradient arrays.  Not const: read at run time, like those.
__device__ float g_ctc_step_seeds[2] = {-1.0f, 1.0f};

// utterance b's pair, from the launch's descriptor and the utterance's staging entry {label offset, U, rows, arc offset}
// (one record serves both sweeps: the forward body reads no gradient field, the backward body neither norm nor em_copy)
__device__ __forceinline__ BandPair step_pair(const CtcStepDesc& d, int b, const gtnx_i4 e) {
  BandPair P;
  const int U = e.y, N = 2 * U + 1;
  GTNX_G char* rec = reinterpret_cast<GTNX_G char*>(d.rec) + int64_t(b) * d.rec_stride;
  P.nodes = reinterpret_cast<const GTNX_G BandNode*>(rec);
  P.nflags = reinterpret_cast<const GTNX_G uint8_t*>(rec + d.o_flags);
  P.snode = reinterpret_cast<const GTNX_G int*>(rec + d.o_snode);
  P.slab = reinterpret_cast<const GTNX_G int*>(rec + d.o_slab);
  P.w = nullptr;
  P.em = reinterpret_cast<const GTNX_G float*>(d.em) + int64_t(b) * d.em_stride;
  P.em_copy = nullptr;
  P.alpha = reinterpret_cast<GTNX_G float*>(d.alpha) + int64_t(b) * d.alpha_stride;
  P.aoff = reinterpret_cast<GTNX_G double*>(d.aoff) + int64_t(b) * d.aoff_stride;
  P.score = reinterpret_cast<GTNX_G float*>(d.score) + b;
  P.rowlse = reinterpret_cast<GTNX_G float*>(d.rowlse) + int64_t(b) * d.T;
  P.norm = reinterpret_cast<GTNX_G float*>(d.norm) + b;
  P.delta = (const GTNX_G float*)g_ctc_step_seeds;
  P.delta_norm = (const GTNX_G float*)(g_ctc_step_seeds + 1);
  P.grad_em = reinterpret_cast<GTNX_G float*>(d.grad) + int64_t(b) * d.em_stride;
  P.grad_fixed = d.tgrad ? reinterpret_cast<GTNX_G float*>(d.tgrad) + e.w : nullptr;
  P.N = N;
  P.T = e.z;
  P.C = d.C;
  P.NS = (N + 3) & ~3;  // band_row_stride
  P.hot = U + 1 >= 8 ? d.blank : -1;
  P.lgrn = d.lgrn;
  P.n_lab = N;
  P.bidx = b;
  P.goff = e.w;
  return P;
}

// The pair as the head left it in LDS, every field in scalar registers.  The sweeps read it from THERE, not from
// step_pair() directly: the bodies were tuned to their register budget with nothing known about a pair at compile
// time (it comes out of a launch's table), and what step_pair() lets the compiler know -- null weights, NS as a
// function of N, the seeds' addresses -- sent the register allocator another way: 7 to 15 vector spills in the
// backward sweep, which sits exactly at its cap of 80 registers.
__device__ __forceinline__ BandPair uniform_pair(const BandPair& s) {
  constexpr int NW = int(sizeof(BandPair) / 4);
  static_assert(sizeof(BandPair) % 4 == 0, "a pair is whole words");
  const int* src = reinterpret_cast<const int*>(&s);
  int w[NW];
#pragma unroll
  for (int i = 0; i < NW; ++i) w[i] = __builtin_amdgcn_readfirstlane(src[i]);
  BandPair P;
  __builtin_memcpy(&P, w, sizeof(BandPair));
  return P;
}

struct StepShared {
  BandPair pair;
  GTNX_G float* loss;
  int lab_off, nsb;
};

// (the kernel's name begins with band_backward_kernel: the profiler family of the launch is band_forward_score_grad,
//  and committed counter passes are looked up by that family's kernel prefix)
template <bool GRADG_, int KF, int KB>
__global__ __launch_bounds__(WGB, 6) void band_backward_kernel_step(CtcStepDesc d, int NSf, int NSb, int tail) {
  constexpr int NPL = 1;
  constexpr bool UNIT = true, VEC = true, BIG = false, GRADG = GRADG_;
  // What the phases share sits in the dynamic block BEHIND the sweeps' carves (`tail` floats in): a static LDS object
  // would shift the dynamic block, and with it every LDS address of the sweeps.  EVERYTHING a later phase needs is read
  // from here, not from the kernel's arguments: a scalar register that lives across the forward sweep is spilled
  // there -- that sweep is short of scalar registers on its own.
  extern __shared__ float lds_all[];
  StepShared& S = *reinterpret_cast<StepShared*>(lds_all + tail);
  // ---------------------------------------------------------------- head: the staging entry, the target records
  {
    extern __shared__ float lds[];
    if (threadIdx.x == 0) {
      const int b = blockIdx.x;
      const gtnx_i4 e = reinterpret_cast<const GTNX_G gtnx_i4*>(d.stage)[b];  // (zero-copy: pinned host memory)
      S.pair = step_pair(d, b, e);
      S.lab_off = e.x;
      S.loss = d.loss + b;
      S.nsb = NSb;
    }
    __syncthreads();
    const BandPair P = uniform_pair(S.pair);
    CtcTargetArgs a;
    a.labels = reinterpret_cast<const GTNX_G int*>(d.labels) + __builtin_amdgcn_readfirstlane(S.lab_off);
    a.nodes = const_cast<GTNX_G BandNode*>(P.nodes);
    a.nflags = const_cast<GTNX_G uint8_t*>(P.nflags);
    a.snode = const_cast<GTNX_G int*>(P.snode);
    a.slab = const_cast<GTNX_G int*>(P.slab);
    a.n_arcs = nullptr;
    a.N = P.N;
    a.pad = 0;
    int* tl = reinterpret_cast<int*>(lds);
    ctc_target_records(a, d.blank, tl, tl + 264);
  }
  // (the records are read by other waves of THIS workgroup -- the same CU, the same vector L1, the same L2: release and
  //  acquire at workgroup scope.  Device scope is what was tried first and is wrong here for speed, not for results: on a
  //  part whose L2 is split over several dies a device-scope release writes the die's L2 back and the acquire invalidates
  //  it, for every workgroup of the launch -- the step took 0.84 ms with them against 0.55 ms through the two sweeps)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  // ---------------------------------------------------------------- forward sweep + normaliser
  {
    constexpr int K = KF;
    const int NSmax = NSf;
#define GTNX_BAND_PAIR uniform_pair(S.pair)
#define GTNX_FWD_IDLE_FROM 8
#include "band_forward_body.inc"
#undef GTNX_FWD_IDLE_FROM
#undef GTNX_BAND_PAIR
  }
  // ---------------------------------------------------------------- hand-over: the loss; alpha rows, shifts, row
  // log-sum-exps and the score become visible to the waves that read them next
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  if (threadIdx.x == 0) {
    const float nrm = S.pair.norm[0], sc = S.pair.score[0];
    S.loss[0] = nrm - sc;  // (vec_axpby_kernel with factors 1 and -1: one rounding)
  }
  // ---------------------------------------------------------------- backward sweep
  {
    constexpr int K = KB;
    const int NSmax = __builtin_amdgcn_readfirstlane(S.nsb);
#define GTNX_BAND_PAIR uniform_pair(S.pair)
#define GTNX_BWD_RS4_LEAN 1
#include "band_backward_body.inc"
#undef GTNX_BWD_RS4_LEAN
#undef GTNX_BAND_PAIR
  }
}

constexpr size_t LDS_TWO = 78 * 1024;

template <bool GRADG, int KF, int KB>
void launch_step3(const CtcStepDesc& d, int n, int nsf, int nsb, size_t lds, int tail, hipStream_t st) {
  static std::atomic<uint64_t> done{0};
  if (gtnx_first_on_device first{done})
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(band_backward_kernel_step<GRADG, KF, KB>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512);
  hipLaunchKernelGGL((band_backward_kernel_step<GRADG, KF, KB>), dim3(n), dim3(WGB), lds, st, d, nsf, nsb, tail);
}
template <int KF, int KB>
void launch_step2(const CtcStepDesc& d, int n, int nsf, int nsb, size_t lds, int tail, bool gradg, hipStream_t st) {
  if (gradg) launch_step3<true, KF, KB>(d, n, nsf, nsb, lds, tail, st);
  else launch_step3<false, KF, KB>(d, n, nsf, nsb, lds, tail, st);
}

struct StepCell {
  int kf, kb, nsb;
  int tail;    // floats in front of the phases' shared record
  size_t lds;  // bytes of the launch's dynamic block
};
// the cell of (C labels, rows of max_NS floats), or kf == 0
StepCell step_cell(int C, int max_NS) {
  StepCell c{0, 0, 0, 0, 0};
  if (C < band_min_labels() || C % 4 != 0 || max_NS <= 0 || max_NS > 256) return c;
  const int kf = band_block_rows(C, 0, false), kb = band_block_rows(C, max_NS, true);
  if (kb == 0 || kf == 0 || kb * C > 1024 || kb * max_NS > 1024) return c;  // (BIG, or no LDS for it)
  if (!((kf == 8 && kb == 4) || (kf == 8 && kb == 2) || (kf == 4 && kb == 2))) return c;
  const int nsb = kb == 4 ? (max_NS + 15) / 16 * 16 : max_NS;  // (band.hip: band_backward_lds_stride)
  // (the sweeps' launchers keep 64 bytes of slack behind a carve; so does this)
  const int tail = ((std::max(band_lds(C, kf, max_NS, false).total, band_lds(C, kb, nsb, true).total) + 3) & ~3) + 16;
  const size_t lds = 4 * size_t(tail) + sizeof(StepShared) + 64;
  if (lds > LDS_TWO) return c;
  c = StepCell{kf, kb, nsb, tail, lds};
  return c;
}

} // namespace

bool ctc_step_cell(int C, int max_NS) { return step_cell(C, max_NS).kf != 0; }

void launch_ctc_step(const CtcStepDesc& d, int n, int max_NS, bool gradg, hipStream_t st) {
  if (n <= 0) return;
  const StepCell c = step_cell(d.C, max_NS);
  if (c.kf == 0) throw std::logic_error("ctc_step.hip: no cell for this shape");
  if (c.kf == 8 && c.kb == 4) launch_step2<8, 4>(d, n, max_NS, c.nsb, c.lds, c.tail, gradg, st);
  else if (c.kf == 8) launch_step2<8, 2>(d, n, max_NS, c.nsb, c.lds, c.tail, gradg, st);
  else launch_step2<4, 2>(d, n, max_NS, c.nsb, c.lds, c.tail, gradg, st);
}

} // namespace gtnx
