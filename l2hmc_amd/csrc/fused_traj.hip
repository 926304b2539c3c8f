// Whole-trajectory persistent kernel for the lattice integrator (gfx950).
//
// One launch integrates ALL leapfrog steps of
//   l2hmc/dynamics/gauge_dynamics.py:261-313 (transition_kernel) with
//   :412-483 (_forward_lf/_backward_lf), :486-590 (sub-updates), :592-609 (accept
//   prob), network/generic_net.py:129-146 (S/T/Q nets) and the U(1) force
//   (:698-709 over lattice/lattice.py:337-362)
// for a tile of 16 chain-rows per workgroup.  Chains are independent and the
// plaquette stencil is local to a chain, so a workgroup never talks to another
// one: x, v, force, both hidden activations and the log-det sums live in LDS
// for the whole trajectory (read from / written to HBM exactly once), and the
// only steady-state traffic is the weight stream.
//
// Why 16 rows: rows / 256 CUs = 16 at the benchmark shape (2 directions x 2048
// chains), which is exactly one 16x16x4 fp32 MFMA tile in M.  Every CU then
// streams every weight once per network call: (2DH + H^2 + 3DH) * 4 B = 2.36 MB
// per 18.9 MFLOP of MFMA work, i.e. ~77 GB/s per CU at the fp32 MFMA peak --
// the L2 -> CU fabric roofline and the MFMA roofline coincide.
// Weights are therefore pre-packed (l2hmc_dense_pack) into the exact order a
// wave consumes them -- [wave][k-chunk][n-tile][lane][4] -- so each B-fragment
// load is one fully coalesced 1 KiB global_load_dwordx4 straight into VGPRs (no
// LDS round trip: a wave's columns are not shared with other waves), double
// buffered one k-chunk (16 k) ahead.  The A operand (16 rows of activations) is
// shared by the 4 waves and read from LDS with conflict-free ds_read_b128
// (row stride = K + 8 floats).
//
// Paired momentum half-kicks (GenericNet sampling instance, 8 waves on the 4-wave image): the second half-kick of
// leapfrog step s and the first of step s + 1 are two VNet evaluations at the same (x, force) that differ only in the
// time term of the first-layer epilogue.  Inside a launch they run as ONE pass: the first layer once, its epilogue
// twice (step s's rows into h1, step s + 1's into h2), then in every image section the even wave walks layer 2 and
// the heads for step s over all of the section's tiles in the reverse direction (as an odd call does) and the odd
// wave does the same for step s + 1 forward -- every accumulator keeps its k order, so the bits do not change -- and
// the odd wave applies its kick to the v' the even wave has written, behind a barrier.  Five barriers and three MFMA
// phases of twice the length instead of seven and five; the next step's masks are loaded inside the pass.
// L2HMC_PLAN_SINGLE_KICKS keeps one network call per half-kick (A/B).  DESIGN.md section 4, K1.
#include "fused_step.h"
#include "lf_update.h"
#include <atomic>
#include <stdlib.h>

namespace l2hmc {

// D = x_dim, H = hidden width, KA = width of each first-layer input (x_dim for GenericNet; the flattened conv
// features for ConvNet3D), CONV = the two inputs go through the conv front-end first (8x8 lattice, F = 8).
template <int D, int H, int KA = D, bool CONV = false>
struct FusedCfg {
  // Waves per workgroup: TWO per SIMD in every instance.  ConvNet3D plans since round 2 (their VALU conv stage is
  // latency-bound at one: 0.987 -> 0.883 ms per step).  The GenericNet kernel used to be faster with one wave per SIMD
  // (rounds 1-3: 1.655 against 1.745 ms); with the weight stream of round 4 (buffer loads, pinned interleave) two win --
  // one wave's epilogues and barriers lie under the other's matrix instructions: 1.431 -> 1.38 ms per step.
  // IMGW: waves the packed weight image is laid out for (pack_fused_kernel).  The 8-wave GenericNet instances read the
  // SAME 4-wave image as the 32-row form and the reverse kernel: two waves share a section (fused_common.h: load_frags),
  // and the taped forward writes its relu-gate words in the 4-wave lane order the reverse kernel reads (fused_train.hip).
  static constexpr int IMGW = CONV ? 2 * kFWaves : kFWaves;
  static constexpr int WAVES = 2 * kFWaves;
  static constexpr int RW = WAVES / IMGW;      // waves per image section
  static constexpr int THREADS = 64 * WAVES;   // wave w owns output columns [w*N/WAVES, (w+1)*N/WAVES)
  // threads per chain in the chain-local passes (force, kinetic energy, observables): their sums are part of the
  // result's bits, so the GenericNet instances keep 16 whatever their wave count (the other threads idle there)
  static constexpr int TPC = CONV ? THREADS / kFM : 16;
  static constexpr int SX = D + 8;             // LDS row stride of x / v / second-input rows
  static constexpr int SA = KA + 8;            // LDS row stride of the conv feature rows
  static constexpr int SH = H + 8;             // LDS row stride of h1 / h2
  static constexpr int NT1 = H / (16 * WAVES);     // 16-column tiles per wave, layers 1 and 2
  static constexpr int NTH = D / (16 * WAVES);     // tiles per wave per head
  static constexpr int NTI1 = H / (16 * IMGW);     // ... and per image section (= NT1, NTH unless two waves share it)
  static constexpr int NTIH = D / (16 * IMGW);
  static_assert(NT1 >= 1 && NT1 <= 8 && NTH >= 1, "every wave needs at least one tile per layer");
  static_assert(RW == 1 || NTH == 1, "a shared heads section is walked with one tile per head and wave");
  static constexpr int KC1 = 2 * KA / 16;      // k-chunks (16 k each), layer 1
  static constexpr int KC2 = H / 16;           // k-chunks, layers 2 and heads
  static constexpr size_t P1 = (size_t)2 * KA * H;  // packed floats per section
  static constexpr size_t P2 = (size_t)H * H;
  static constexpr size_t PH = (size_t)3 * D * H;
  // per-net constants kept in LDS: b1[H] wt[2H] bh[H] bhd[3D] exp(cs)[D] exp(cq)[D]
  static constexpr int NC = 4 * H + 5 * D;
  // conv front-end (CONV only): F = 8 filters on the 8x8 lattice
  static constexpr int CF = 8, CL = 8;
  static constexpr int CW = 18 * CF + CF + 8 * CF * CF + 2 * CF;            // one (net, input) filter set
  static constexpr int CXIN = (CL + 2) * (CL + 2) * 2;                      // haloed chain
  static constexpr int CP1 = (CL / 2 + 1) * (CL / 2 + 1) * CF;              // pooled conv1 map, zero halo
  static constexpr int CONV_FLOATS = CONV ? 2 * kFM * SA + 4 * CW + kFM * (CXIN + CP1) : 0;
  // active-column heads (GenericNet, split step mode): log-det terms staged at their columns [16][SX], the two
  // column lists of this workgroup's mask row [2][D / 2] (int) and their eligibility [2] (int, padded to 4); the
  // kept-column first layer's column -> compact k map [D] (int) and its per-row poison values [2][16]
  static constexpr int ACT_FLOATS = CONV ? 0 : kFM * SX + D + 4 + D + 2 * kFM;
  static constexpr int LDS_FLOATS = 3 * kFM * SX + 2 * kFM * SH + 2 * NC + kFM * (D / 2 + 4) /*sinP*/ +
                                    2 * D /*masks*/ + WAVES * kFM /*ldw*/ + (RW > 1 ? IMGW * 64 : 0) /*ldx*/ + kFM /*dir*/ +
                                    8 * kFM /*step mode*/ + CONV_FLOATS + ACT_FLOATS;
};

// ---------------------------------------------------------------------------
// weight packing (device side, once per weight update)
// ---------------------------------------------------------------------------
__global__ void pack_fused_kernel(l2hmc_dense_net n, float* __restrict__ out, int waves) {
  const int kFWaves = waves;                 // waves per workgroup of the kernel that will read this image
  const int D = n.D, H = n.H, K1 = n.Ka + n.Kb;
  const size_t P1 = (size_t)K1 * H, P2 = (size_t)H * H, PH = (size_t)3 * D * H;
  const int NT1 = H / (16 * kFWaves), NTH = D / (16 * kFWaves);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < P1 + P2 + PH;
       i += (size_t)gridDim.x * blockDim.x) {
    const int j = (int)(i & 3), lane = (int)((i >> 2) & 63);
    size_t rest;
    float val;
    if (i < P1 + P2) {
      const bool first = i < P1;
      const int K = first ? K1 : H;
      rest = (first ? i : i - P1) >> 8;               // ((w * KC + kc) * NT1 + t)
      const int t = (int)(rest % NT1);
      rest /= NT1;
      const int KC = K / 16;
      const int kc = (int)(rest % KC), w = (int)(rest / KC);
      const int col = (w * NT1 + t) * 16 + (lane & 15);
      const int k = kc * 16 + (lane >> 4) * 4 + j;
      val = first ? n.w1_t[(size_t)col * K1 + k] : n.wh_t[(size_t)col * H + k];
    } else {
      rest = (i - P1 - P2) >> 8;                      // (((w * KC2 + kc) * 3 + hd) * NTH + t)
      const int t = (int)(rest % NTH);
      rest /= NTH;
      const int hd = (int)(rest % 3);
      rest /= 3;
      const int KC = H / 16;
      const int kc = (int)(rest % KC), w = (int)(rest / KC);
      const int col = w * (D / kFWaves) + t * 16 + (lane & 15);
      const int k = kc * 16 + (lane >> 4) * 4 + j;
      val = n.whd_t[((size_t)hd * D + col) * H + k];
    }
    out[i] = val;
  }
}

// Active-column heads sections (l2hmc_gauge_pack_heads): block (x, 2 m + sense) lists the columns of mask row m
// that a position sub-update with keep = mask (sense 0) or keep = 1 - mask (sense 1) moves, records whether the row
// qualifies (every entry exactly 0 or 1, D / 2 of them moving) and packs XNet's heads for those columns in the order
// of the 4-wave image -- [section = active tile][k-chunk][head][lane][4] -- one 16-column tile per section.
// Kept-column first layer: the same block packs the x-half of XNet's W1 for the D / 2 columns that sub-update KEEPS
// (its second input keep (.) x is exactly zero everywhere else) as a first-layer image of D / 2 k -- [section]
// [chunk 0..D/32-1][tile][lane][4].  A 16-k chunk is walked e-major (k = 4 q + e: e = 0..3 outer, q = 0..3 inner), so
// the n-th kept column of that walk over all D columns takes the compact k whose turn is n-th in the compact walk:
// every accumulator meets its kept columns in today's order (kept_compact_k).
__host__ __device__ inline int kept_compact_k(int n) { return (n & ~15) + 4 * (n & 3) + ((n >> 2) & 3); }

__global__ __launch_bounds__(256) void pack_heads_kernel(l2hmc_dense_net n, const float* __restrict__ masks, int N,
                                                         int* __restrict__ meta, float* __restrict__ img,
                                                         int* __restrict__ cpos, float* __restrict__ img1) {
  constexpr int DMAX = 128;
  __shared__ int cols[DMAX / 2];
  __shared__ int kcol[DMAX / 2];          // compact k -> kept column
  __shared__ int ok;
  const int D = n.D, H = n.H, DA = D / 2, K1 = n.Ka + n.Kb;
  const float* row = masks + (size_t)(blockIdx.y >> 1) * D;
  const float sense = (float)(blockIdx.y & 1);
  if (threadIdx.x == 0) {
    int cnt = 0, bin = D <= DMAX;
    for (int c = 0; c < D && bin; ++c) {
      const float v = row[c];
      if (!(v == 0.f || v == 1.f)) bin = 0;
      else if (v == sense) {
        if (cnt < DA) cols[cnt] = c;
        ++cnt;
      }
    }
    ok = bin && cnt == DA;
    if (ok) {
      int nk = 0;
      for (int w = 0; w < D; ++w) {                   // the full walk: chunk, e, q
        const int c = (w & ~15) + 4 * (w & 3) + ((w >> 2) & 3);
        if (row[c] != sense) kcol[kept_compact_k(nk++)] = c;
      }
    }
  }
  __syncthreads();
  if (blockIdx.x == 0) {
    if (threadIdx.x == 0) meta[blockIdx.y] = ok;
    for (int i = threadIdx.x; i < DA; i += blockDim.x) meta[2 * N + (size_t)blockIdx.y * DA + i] = ok ? cols[i] : -1;
    // column -> compact k of the sub-update that keeps it (each block fills in the columns it keeps)
    int* cp = cpos + (size_t)(blockIdx.y >> 1) * D;
    if (ok) {
      for (int i = threadIdx.x; i < DA; i += blockDim.x) cp[kcol[i]] = i;
    } else {
      for (int i = threadIdx.x; i < D; i += blockDim.x) cp[i] = -1;
    }
  }
  if (!ok) return;
  const size_t per = (size_t)3 * DA * H;
  float* out = img + (size_t)blockIdx.y * per;
  const int KC = H / 16;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < per; i += (size_t)gridDim.x * blockDim.x) {
    const int j = (int)(i & 3), lane = (int)((i >> 2) & 63);
    size_t rest = i >> 8;                             // ((w * KC + kc) * 3 + hd)
    const int hd = (int)(rest % 3);
    rest /= 3;
    const int kc = (int)(rest % KC), w = (int)(rest / KC);
    const int col = cols[w * 16 + (lane & 15)];
    const int k = kc * 16 + (lane >> 4) * 4 + j;
    out[i] = n.whd_t[((size_t)hd * D + col) * H + k];
  }
  const size_t per1 = (size_t)DA * H;
  float* out1 = img1 + (size_t)blockIdx.y * per1;
  const int KC1 = DA / 16, NT = H / (16 * 4);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < per1; i += (size_t)gridDim.x * blockDim.x) {
    const int j = (int)(i & 3), lane = (int)((i >> 2) & 63);
    size_t rest = i >> 8;                             // ((w * KC1 + kc) * NT + t)
    const int t = (int)(rest % NT);
    rest /= NT;
    const int kc = (int)(rest % KC1), w = (int)(rest / KC1);
    const int col = (w * NT + t) * 16 + (lane & 15);
    const int k = kc * 16 + (lane >> 4) * 4 + j;
    out1[i] = n.w1_t[(size_t)col * K1 + n.Ka + kcol[k]];
  }
}

// (struct FusedArgs: fused_args.h, shared with the sub-tile form in fused_traj4.hip)

#ifdef L2HMC_STAMPS
int g_fused_stagger = 0;
extern "C" void l2hmc_debug_set_stagger(int cycles) { g_fused_stagger = cycles; }
#endif

// TAPE: training instantiation (GenericNet plans) that also writes the per-call tape of train.hip
// LADDER: step mode with a beta per chain (FusedArgs::step_betas), an instance of its own next to the sampling one
// TAPE && LADDER: the taped forward of a training step on a ladder (trajectory mode, a beta per row; fused_step.h)
template <int D, int H, int KA, bool CONV, bool TAPE = false, bool LADDER = false>
__global__ __launch_bounds__((FusedCfg<D, H, KA, CONV>::THREADS)) void gauge_traj_fused_kernel(FusedArgs p) {
  using Cfg = FusedCfg<D, H, KA, CONV>;
  constexpr int kFWaves = Cfg::WAVES, kFThreads = Cfg::THREADS, kTPC = Cfg::TPC;   // this instance's geometry
  constexpr int SX = Cfg::SX, SH = Cfg::SH, SA = Cfg::SA, NT1 = Cfg::NT1, NTH = Cfg::NTH;
  constexpr int RW = Cfg::RW, IMGW = Cfg::IMGW, NTI1 = Cfg::NTI1, NTIH = Cfg::NTIH;
  constexpr int TSH = RW > 1 ? NTIH : 1;       // tile stride of a wave's heads fragments in a shared section
  constexpr int sites = D / 2;
  constexpr int SP = sites + 4;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xs = lds;                         // [16][SX] position
  float* vs = xs + kFM * SX;               // [16][SX] momentum
  float* gs = vs + kFM * SX;               // [16][SX] second net input: force, or keep (.) x
  float* h1 = gs + kFM * SX;               // [16][SH]
  float* h2 = h1 + kFM * SH;               // [16][SH]
  float* cx = h2 + kFM * SH;               // XNet constants [NC]
  float* cv = cx + Cfg::NC;                // VNet constants [NC]
  float* sp = cv + Cfg::NC;                // [16][SP] sin P
  float* skm = sp + kFM * SP;              // [2][D]  masks of this step: forward row, backward row
  float* ldw = skm + 2 * D;                // [IMGW][16] log-det partial sums per image wave; behind them (RW > 1 only)
                                           // [IMGW][64] the lane sums an even wave hands to its odd partner
  float* ldx = ldw + IMGW * kFM;
  int* sdir = reinterpret_cast<int*>(ldw + kFWaves * kFM + (RW > 1 ? IMGW * 64 : 0));   // [16]
  float* stp = reinterpret_cast<float*>(sdir + kFM);  // step mode: coin[16] u[16] p_row[16] obs[16][4] beta[16]
  // ConvNet3D front-end state (CONV only; zero-sized otherwise)
  float* fa = stp + 8 * kFM;                          // [16][SA] features of the first input
  float* fb = fa + kFM * SA;                          // [16][SA] features of the second input
  float* cwl = fb + kFM * SA;                         // [net x|v][input a|b][CW] filters
  float* cxin = cwl + 4 * Cfg::CW;                    // [16][CXIN] haloed chains
  float* cp1 = cxin + kFM * Cfg::CXIN;                // [16][CP1]  pooled conv1 maps
  // active-column heads (GenericNet only; zero-sized otherwise)
  float* stg = stp + 8 * kFM + Cfg::CONV_FLOATS;      // [16][SX] log-det terms of a position call at their columns
  int* scol = reinterpret_cast<int*>(stg + kFM * SX);  // [2][D / 2] active columns of keep sense 0 / 1, ascending
  int* sel = scol + D;                                 // [2] the two lists are usable (exactly D / 2 columns, 0 / 1 mask)
  int* scp = sel + 4;                                  // [D] column -> compact k of the position sub-update that keeps it
  float* spz = reinterpret_cast<float*>(scp + D);      // [2][16] NaN: the row's next sub-update (1st, 2nd) sees 0 x non-finite

  // diagnostic cycle shares: 0-2 gemm L1/L2/heads, 3-5 their epilogues, 6 barriers, 7 force, 8 mask pass, 9 total
  [[maybe_unused]] unsigned long long ft[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  [[maybe_unused]] const unsigned long long ft_start = L2HMC_CYCLES_NOW();
#ifdef L2HMC_STAMPS
  unsigned long long rt0;
  asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rt0)::"memory");
#endif
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int q = lane >> 4, r = lane & 15;
  const int64_t row0 = (int64_t)blockIdx.x * kFM;
  const int nrow = (int)min((int64_t)kFM, p.rows - row0);
  const float eps = p.eps;

#ifdef L2HMC_STAMPS
  if (p.stagger > 0) {
    // (diagnostic build) spread the workgroups of an XCD (blockIdx & 7 labels the XCD group) over the weight stream
    const long long delay = (long long)((blockIdx.x >> 3) & 31) * p.stagger;
    const long long t0 = (long long)__builtin_amdgcn_s_memtime();
    while ((long long)__builtin_amdgcn_s_memtime() - t0 < delay) __builtin_amdgcn_s_sleep(16);
  }
#endif
  // ---- stage chain state and constants (fused_step.h) ----------------------------
  // split step mode (FusedArgs::step_split): 16 chains of one direction, the direction uniform over the workgroup
  const bool SPLIT = !CONV && !TAPE && p.step_B > 0 && p.step_both && p.step_split;
  const StepWg wg = step_workgroup<kFM>(p, stp, SPLIT);
  const bool STEPM = wg.stepm;
  const int sdw = wg.sdw;                                               // (SPLIT) this workgroup's direction
  float* spx = wg.spx;                                                  // [16] accept probability per row
  stage_chains<kFM, kFThreads, D, SX, LADDER, TAPE>(p, wg, xs, vs, sdir);
  load_consts<kFThreads, D, H>(p.xnet, cx, tid);
  load_consts<kFThreads, D, H>(p.vnet, cv, tid);
  if constexpr (CONV) {
    constexpr int F = Cfg::CF, F2 = 2 * Cfg::CF;
    auto load_filters = [&](const float* w1, const float* b1, const float* w2, const float* b2, float* dst) {
      for (int i = tid; i < 18 * F; i += kFThreads) dst[i] = w1[i];
      for (int i = tid; i < F; i += kFThreads) dst[18 * F + i] = b1[i];
      for (int i = tid; i < 4 * F * F2; i += kFThreads) {      // Keras [di][dj][dd][c][g]: keep dd = 0
        const int g = i % F2, c = (i / F2) % F, tap = i / (F2 * F);
        dst[19 * F + i] = w2[((size_t)(tap * 2) * F + c) * F2 + g];
      }
      for (int i = tid; i < F2; i += kFThreads) dst[19 * F + 4 * F * F2 + i] = b2[i];
    };
    load_filters(p.xfront.w1_a, p.xfront.b1_a, p.xfront.w2_a, p.xfront.b2_a, cwl + 0 * Cfg::CW);
    load_filters(p.xfront.w1_b, p.xfront.b1_b, p.xfront.w2_b, p.xfront.b2_b, cwl + 1 * Cfg::CW);
    load_filters(p.vfront.w1_a, p.vfront.b1_a, p.vfront.w2_a, p.vfront.b2_a, cwl + 2 * Cfg::CW);
    load_filters(p.vfront.w1_b, p.vfront.b1_b, p.vfront.w2_b, p.vfront.b2_b, cwl + 3 * Cfg::CW);
    for (int i = tid; i < kFM * (Cfg::CXIN + Cfg::CP1); i += kFThreads) cxin[i] = 0.f;   // halos stay zero
  }
  if (tid < IMGW * kFM) ldw[tid] = 0.f;
  if constexpr (!CONV) {
    if (tid < 2 * kFM) spz[tid] = 0.f;
  }
  __syncthreads();

  const int dirl = sdir[r];           // direction of the row this lane owns in a C fragment (fused_common.h)

  // ---- chain-local passes (fused_step.h): kTPC consecutive threads per chain, one chain per thread group
  const ChainLanes cl = chain_lanes<kFM, kTPC, 1>(p, wg, tid);
  float act0[1], kin0[1];
  force_pass<kFM, kTPC, 1, D, SX, SP, LADDER>(cl, xs, sp, gs, act0);     // also leaves the force of x0 in gs
  kinetic_pass<kFM, kTPC, 1, D, SX>(cl, vs, kin0);

  // ---- one network evaluation + fused sub-update ------------------------------
  // in1: first input rows (LDS, stride SX); second input is always gs.
  // mode 1: momentum update (uses gs as the force), mode 2: position update with keep masks.
  // ConvNet3D front-end on a [16][SX] LDS array (network/conv_net.py:251-262; same arithmetic as
  // conv3d_front_kernel): conv1(3,3,2)+relu+pool -> cp1, conv2(2,2,[2])+relu+pool -> dst [16][SA].
  [[maybe_unused]] auto conv_features = [&](const float* src, const float* cw, float* dst) {
    constexpr int F = Cfg::CF, F2 = 2 * Cfg::CF, L = Cfg::CL, LP = L + 2, L2 = L / 2, L2P = L2 + 1, L4 = L / 4;
    const float* w1 = cw;
    const float* b1 = cw + 18 * F;
    const float* w2 = b1 + F;
    const float* b2 = w2 + 4 * F * F2;
    for (int i = tid; i < kFM * D; i += kFThreads) {
      const int c = i / D, e = i - c * D;
      const int site = e >> 1, mu = e & 1, ii = site / L, jj = site - ii * L;
      cxin[c * Cfg::CXIN + ((ii + 1) * LP + jj + 1) * 2 + mu] = src[c * SX + e];
    }
    __syncthreads();
    // conv1 + relu + pool.  A thread owns a PAIR of filters (2 fp, 2 fp + 1) of one pooled position: the pair's 18
    // taps sit in registers for all of its positions (the workgroup size is a multiple of F / 2, so fp never
    // changes), the 4 x 4 x 2 input patch under the 2 x 2 pooling window is read once (16 ds_read_b64 instead of
    // 72 + 72 scalar reads), and every multiply-add is a v_pk_fma_f32 over the filter pair.
    {
      using f32x2 = __attribute__((ext_vector_type(2))) float;
      constexpr int FP = F / 2;
      static_assert(kFThreads % FP == 0 && F % 2 == 0, "filter pairs must stay with their threads");
      const int fp = tid % FP;
      f32x2 k0[9], k1[9];
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        k0[t] = *reinterpret_cast<const f32x2*>(w1 + (t * 2 + 0) * F + 2 * fp);
        k1[t] = *reinterpret_cast<const f32x2*>(w1 + (t * 2 + 1) * F + 2 * fp);
      }
      const f32x2 bias = *reinterpret_cast<const f32x2*>(b1 + 2 * fp);
      for (int idx = tid; idx < kFM * L2 * L2 * FP; idx += kFThreads) {
        int rr = idx / FP;
        const int J = rr % L2;
        rr /= L2;
        const int I = rr % L2, c = rr / L2;
        f32x2 px[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int bb = 0; bb < 4; ++bb)
            px[a][bb] = *reinterpret_cast<const f32x2*>(cxin + c * Cfg::CXIN + ((2 * I + a) * LP + 2 * J + bb) * 2);
        f32x2 m = {-INFINITY, -INFINITY};
#pragma unroll
        for (int a = 0; a < 2; ++a) {
#pragma unroll
          for (int bb = 0; bb < 2; ++bb) {
            f32x2 v0 = bias, v1 = bias;              // the two depth positions of conv_net.py's (3, 3, 2) filter
#pragma unroll
            for (int di = 0; di < 3; ++di) {
#pragma unroll
              for (int dj = 0; dj < 3; ++dj) {
                const f32x2 xx = px[a + di][bb + dj];
                const f32x2 x0 = {xx[0], xx[0]}, x1 = {xx[1], xx[1]};
                v0 += x0 * k0[di * 3 + dj];      // (conv3d_front.hip's order: three fused multiply-adds per tap)
                v0 += x1 * k1[di * 3 + dj];
                v1 += x1 * k0[di * 3 + dj];
              }
            }
            m[0] = max_nan(m[0], max_nan(v0[0], v1[0]));
            m[1] = max_nan(m[1], max_nan(v0[1], v1[1]));
          }
        }
        *reinterpret_cast<f32x2*>(cp1 + c * Cfg::CP1 + (I * L2P + J) * F + 2 * fp) = f32x2{relu_nan(m[0]), relu_nan(m[1])};
      }
    }
    __syncthreads();
    // conv2 + relu + pool, again a pair of filters (2 gp, 2 gp + 1) per thread: the 2 x 2 outputs of the pooling
    // window share a 3 x 3 patch of the pooled conv1 map -- per 4 input channels, 9 ds_read_b128 (patch) + 16
    // ds_read_b64 (taps of the pair) feed 64 v_pk_fma_f32
    {
      using f32x2 = __attribute__((ext_vector_type(2))) float;
      constexpr int GP = F2 / 2;
      for (int idx = tid; idx < kFM * L4 * L4 * GP; idx += kFThreads) {
        const int gp = idx % GP;
        int rr = idx / GP;
        const int J2 = rr % L4;
        rr /= L4;
        const int I2 = rr % L4, c = rr / L4;
        const f32x2 bias = *reinterpret_cast<const f32x2*>(b2 + 2 * gp);
        f32x2 acc[2][2] = {{bias, bias}, {bias, bias}};
        const float* pbase = cp1 + c * Cfg::CP1 + ((2 * I2) * L2P + 2 * J2) * F;
        for (int ch4 = 0; ch4 < F; ch4 += 4) {
          f32x4 w[3][3];
#pragma unroll
          for (int wi = 0; wi < 3; ++wi)
#pragma unroll
            for (int wj = 0; wj < 3; ++wj)
              w[wi][wj] = *reinterpret_cast<const f32x4*>(pbase + (wi * L2P + wj) * F + ch4);
#pragma unroll
          for (int di = 0; di < 2; ++di)
#pragma unroll
            for (int dj = 0; dj < 2; ++dj)
#pragma unroll
              for (int cc = 0; cc < 4; ++cc) {
                const f32x2 kw = *reinterpret_cast<const f32x2*>(w2 + ((di * 2 + dj) * F + ch4 + cc) * F2 + 2 * gp);
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                  for (int bb = 0; bb < 2; ++bb) {
                    const float xv = w[a + di][bb + dj][cc];
                    acc[a][bb] += f32x2{xv, xv} * kw;
                  }
              }
        }
        const float m0 = max_nan(max_nan(acc[0][0][0], acc[0][1][0]), max_nan(acc[1][0][0], acc[1][1][0]));
        const float m1 = max_nan(max_nan(acc[0][0][1], acc[0][1][1]), max_nan(acc[1][0][1], acc[1][1][1]));
        *reinterpret_cast<f32x2*>(dst + c * SA + (I2 * L4 + J2) * F2 + 2 * gp) = f32x2{relu_nan(m0), relu_nan(m1)};
      }
    }
    __syncthreads();
  };

  // First-layer pre-activations that recur unchanged and are kept in registers instead of being recomputed
  // (bit-identical results, 8.3 % fewer weight bytes and MFMAs per leapfrog step):
  //   keep_v: VNet's whole first-layer product.  The second half-kick of step s and the first half-kick of
  //           step s+1 see the same (x, force); only the time term differs, and that is added in the epilogue.
  //   keep_x: XNet's product with its FIRST input (v), identical for the two position sub-updates of a step.
  // keep_x lives from call 1 to call 2 of a step and keep_v from call 3 to the next step's call 0: never both, so
  // the instance with the paired call (below), which needs the registers, keeps them in ONE set.
  constexpr bool KEEP1 = !CONV && !TAPE && Cfg::NTH == 1 && RW == 2 && kFWaves == 8;
  f32x4 keep_v[NT1];
  [[maybe_unused]] f32x4 keep_x_own[KEEP1 ? 1 : NT1];
  f32x4 (&keep_x)[NT1] = *[&]() {
    if constexpr (KEEP1) return &keep_v;
    else return &keep_x_own;
  }();
  bool keep_v_valid = false;
  // Active-column heads (split step mode, l2hmc_gauge_pack_heads): a position sub-update moves only the columns whose
  // keep is 0 -- x' = keep x + (1 - keep) upd and the log-det term carry (1 - keep) -- so S / T / Q are formed for those
  // D / 2 columns alone, from a heads section packed per (mask row, keep sense): 4 tiles x [S | T | Q], one tile per
  // SIMD (waves 0-3; their SIMD partners 4-7 fill in the kept columns' zeros).  Same k order per column, same
  // epilogue expressions; the log-det terms are staged at their columns and summed in today's grouping.
  constexpr bool ACTOK = !CONV && !TAPE && Cfg::NTH == 1 && RW == 2 && kFWaves == 8;
  int arow = 0;                        // mask row of this workgroup's direction at the current step
  // Paired momentum half-kicks (8 waves on the 4-wave image, sampling only): call 3 of step s and call 0 of step s + 1
  // run as ONE pass over two time slices (net_update's `pair`)
  constexpr bool PAIROK = !CONV && !TAPE && Cfg::NTH == 1 && RW == 2 && kFWaves == 8;

  // l1: 0 = compute both halves; 1 = as 0 and store the raw product in keep_v; 2 = take keep_v, no GEMM;
  //     3 = compute, snapshot the first-input half into keep_x; 4 = start from keep_x, second half only.
  auto net_update = [&](const l2hmc_dense_net& net, const float* cn, const float* in1, int mode, int sub,
                        bool prep_next_mask, int l1, bool is_vnet, const float tcr, const float tsr,
                        int callidx, bool pair, const float tcr2, const float tsr2) {
    const float* pk = net.packed;
    // layers 2 and 3 of a network are streamed in alternating directions on its consecutive calls (fused_common.h)
    const bool zig = (callidx & 1) != 0;
    // training tape (generic plans): this call's inputs and the state its sub-update consumes
    [[maybe_unused]] const FusedTape& tp = is_vnet ? p.tv : p.tx;
    [[maybe_unused]] const size_t tcr0 = (size_t)callidx * (size_t)p.rows + (size_t)row0;     // first taped row of this workgroup
    if constexpr (TAPE) {
      {
        const float* stsrc = mode == 1 ? vs : xs;
        for (int i = tid; i < kFM * (D / 4); i += kFThreads) {
          const int rr = i / (D / 4), c4 = (i - rr * (D / 4)) * 4;
          if (rr < nrow) {
            float* dst = tp.in + (tcr0 + rr) * (2 * D);
            tape_store(dst + c4, *reinterpret_cast<const f32x4*>(in1 + rr * SX + c4));
            tape_store(dst + D + c4, *reinterpret_cast<const f32x4*>(gs + rr * SX + c4));
            tape_store(tp.st + (tcr0 + rr) * D + c4, *reinterpret_cast<const f32x4*>(stsrc + rr * SX + c4));
          }
        }
      }
    }
    [[maybe_unused]] auto tape_rows = [&](float* dst, const float* src) {     // [16][H] LDS rows -> tape
      for (int i = tid; i < kFM * (H / 4); i += kFThreads) {
        const int rr = i / (H / 4), c4 = (i - rr * (H / 4)) * 4;
        if (rr < nrow)
          tape_store(dst + (tcr0 + rr) * H + c4, *reinterpret_cast<const f32x4*>(src + rr * SH + c4));
      }
    };
    const int wv = __builtin_amdgcn_readfirstlane(wave);      // provably uniform: the weight loads' base stays in SGPRs
    const int wimg = wv / RW, wsub = wv - wimg * RW;          // image section, and this wave's share of it
    const float* wp1 = pk + (size_t)wimg * Cfg::KC1 * NTI1 * 256;
    const float* wp2 = pk + Cfg::P1 + (size_t)wimg * Cfg::KC2 * NTI1 * 256;
    const float* wph = pk + Cfg::P1 + Cfg::P2 + (size_t)wimg * Cfg::KC2 * 3 * NTIH * 256;
    const int to1 = wsub * NT1, toh = wsub * NTH;             // first tile of this wave in a chunk of the section
    int asense = 0;                                           // keep sense whose columns move: keep = mask (0) / 1 - mask (1)
    bool actv = false;
    const float* wpa = nullptr;
    if (ACTOK && SPLIT && mode == 2 && p.heads_img) {
      asense = sdw ^ sub;
      actv = __builtin_amdgcn_readfirstlane(sel[asense]) != 0;
      wpa = p.heads_img + ((size_t)(arow * 2 + asense) * 4 + (wv & 3)) * Cfg::KC2 * 3 * 256;
    }
    // Kept-column first layer (split step mode, eligible mask row, l2hmc_gauge_pack_heads): the second input of a
    // position sub-update, keep (.) x, is exactly zero in the D / 2 columns the sub-update moves, so its product is
    // formed over the D / 2 kept columns alone, from a first-layer section packed per (mask row, keep sense).  The
    // kept values sit at compact k (scp) in stg (first sub-update; gs still holds the force when they are written) or
    // gs (second); a moving column that would have put 0 x non-finite = NaN into the product raises the row's poison.
    const bool l1c = ACTOK && SPLIT && p.l1_img && p.heads_img && __builtin_amdgcn_readfirstlane(sel[0] & sel[1]) != 0;
    [[maybe_unused]] float ld_k[4] = {0.f, 0.f, 0.f, 0.f}, ld_s[4] = {0.f, 0.f, 0.f, 0.f};   // (RW > 1: the odd wave's log-det terms)
#ifndef L2HMC_DP1                                 // (A/B builds: tools/build_variant.sh)
#define L2HMC_DP1 3
#define L2HMC_DP2 3
#define L2HMC_DPH 4
#endif
    constexpr int DP1 = L2HMC_DP1, DP2 = L2HMC_DP2, DPH = L2HMC_DPH;   // ring depths (fused_common.h): first-layer halves, layer 2, heads
    BRing<NT1, DP2> R2;
    BRing<3 * NTH, DPH> R3;
    // paired call: a wave walks ALL tiles of its image section for one time slice (layer 2: NTI1, heads: 3 NTIH)
#ifndef L2HMC_DP2P
#define L2HMC_DP2P 2
#define L2HMC_DPHP 3
#endif
    constexpr int DP2P = L2HMC_DP2P, DPHP = L2HMC_DPHP;
    [[maybe_unused]] BRing<NTI1, DP2P> R2P;
    [[maybe_unused]] BRing<3 * NTIH, DPHP> R3P;
    // ----- layer 1: two half-K streams (first input rows, then the second-input rows in gs)
    {
      constexpr int KH = Cfg::KC1 / 2;
      f32x4 acc[NT1];
      [[maybe_unused]] unsigned long long t0 = L2HMC_CYCLES_NOW();
      // inputs of the dense trunk: the LDS rows themselves, or their conv features
      const float* src1 = in1;
      const float* src2 = gs;
      int s1 = SX;
      if constexpr (CONV) {
        const float* cwn = cwl + (is_vnet ? 2 : 0) * Cfg::CW;
        [[maybe_unused]] const unsigned long long tc0 = L2HMC_CYCLES_NOW();
        if (l1 == 0 || l1 == 1 || l1 == 3) conv_features(in1, cwn, fa);            // first input (conv_v*)
        if (l1 != 2) conv_features(gs, cwn + Cfg::CW, fb);                          // second input (conv_x*)
        L2HMC_CYCLES_ADD(ft, 8, tc0);               // (slot 8: conv front-end; also inside slot 0)
        src1 = fa;
        src2 = fb;
        s1 = SA;
        if constexpr (TAPE) {      // features (also the reused ones still sitting in fa / fb) -> tape, for d loss / d W1
          for (int i = tid; i < kFM * (2 * KA / 4); i += kFThreads) {
            const int rr = i / (2 * KA / 4), c4 = (i - rr * (2 * KA / 4)) * 4;
            if (rr < nrow)
              tape_store(tp.feat + (tcr0 + rr) * (2 * KA) + c4,
                         *reinterpret_cast<const f32x4*>((c4 < KA ? fa + rr * SA + c4 : fb + rr * SA + (c4 - KA))));
          }
        }
      }
      if (l1 == 2) {
#pragma unroll
        for (int t = 0; t < NT1; ++t) acc[t] = keep_v[t];
      } else {
        BRing<NT1, DP1> RA, RB;
        const bool cmp = l1c && mode == 2;
        const float* wpb = wp1 + (size_t)KH * NTI1 * 256;
        if (cmp) wpb = p.l1_img + ((size_t)(arow * 2 + asense) * IMGW + wimg) * (KH / 2) * NTI1 * 256;
        ring_prime<NT1, DP1, NTI1>(RB, wpb, false, 0, to1);          // both halves' first fragments are requested up front
        if (l1 == 4) {
#pragma unroll
          for (int t = 0; t < NT1; ++t) acc[t] = keep_x[t];
        } else {
          ring_prime<NT1, DP1, NTI1>(RA, wp1, false, 0, to1);
#pragma unroll
          for (int t = 0; t < NT1; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
          const float* a1 = src1 + r * s1 + q * 4;
          stream_layer<NT1, KH, DP1, NTI1>(
              RA, wp1, [&](int kc) { return *reinterpret_cast<const f32x4*>(a1 + kc * 16); }, acc, false, to1);
          if (l1 == 3) {
#pragma unroll
            for (int t = 0; t < NT1; ++t) keep_x[t] = acc[t];
          }
        }
        bool x_done = false;
        if constexpr (ACTOK) {
          if (cmp) {
            x_done = true;
            const float* a2 = (sub == 0 ? stg : gs) + r * SX + q * 4;
            const bool bad = spz[sub * kFM + r] != 0.f;
            stream_layer<NT1, KH / 2, DP1, NTI1>(
                RB, wpb,
                [&](int kc) {
                  f32x4 a = *reinterpret_cast<const f32x4*>(a2 + kc * 16);
                  if (kc == 0) {       // a select, not an add: finite rows keep their bits
#pragma unroll
                    for (int e = 0; e < 4; ++e) a[e] = bad ? __builtin_nanf("") : a[e];
                  }
                  return a;
                },
                acc, false, to1);
          }
        }
        if (!x_done) {
          const float* a2 = src2 + r * s1 + q * 4;
          stream_layer<NT1, KH, DP1, NTI1>(
              RB, wpb, [&](int kc) { return *reinterpret_cast<const f32x4*>(a2 + kc * 16); }, acc, false, to1);
        }
        if (l1 == 1 && !(PAIROK && pair)) {        // (a paired call spends the product at once, on both time terms)
#pragma unroll
          for (int t = 0; t < NT1; ++t) keep_v[t] = acc[t];
        }
      }
      if constexpr (PAIROK) {
        if (pair) {
          // ----- paired call (a path of its own from here on: the single calls' code below stays as it is).  The first
          //       layer's product gets both steps' time terms: slice A (this step's second half-kick) into the h1 rows,
          //       slice B (the next step's first half-kick) into the h2 rows, with the single calls' statement.
          ring_prime<NTI1, DP2P, NTI1, 1>(R2P, wp2, wsub == 0, Cfg::KC2, 0);
          L2HMC_CYCLES_ADD(ft, 0, t0);
          t0 = L2HMC_CYCLES_NOW();
#pragma unroll
          for (int t = 0; t < NT1; ++t) {
            const int c0 = (wave * NT1 + t) * 16 + q * 4;          // this lane: row r, columns c0 .. c0 + 3
            const f32x4 b = *reinterpret_cast<const f32x4*>(cn + c0);
            const f32x4 w0 = *reinterpret_cast<const f32x4*>(cn + H + c0);
            const f32x4 w1 = *reinterpret_cast<const f32x4*>(cn + 2 * H + c0);
            f32x4 hv;
#pragma unroll
            for (int e = 0; e < 4; ++e) hv[e] = relu_nan(acc[t][e] + b[e] + (tcr * w0[e] + tsr * w1[e]));
            *reinterpret_cast<f32x4*>(h1 + r * SH + c0) = hv;
#pragma unroll
            for (int e = 0; e < 4; ++e) hv[e] = relu_nan(acc[t][e] + b[e] + (tcr2 * w0[e] + tsr2 * w1[e]));
            *reinterpret_cast<f32x4*>(h2 + r * SH + c0) = hv;
          }
          L2HMC_CYCLES_ADD(ft, 3, t0);
          {
            [[maybe_unused]] const unsigned long long tb = L2HMC_CYCLES_NOW();
            __syncthreads();
            L2HMC_CYCLES_ADD(ft, 6, tb);
          }
          // The even wave of a section takes slice A (the reverse walk of an odd call), the odd wave slice B (forward
          // walk), each over ALL tiles of the section: every accumulator sees the chunks and the direction it sees in
          // the single calls.  Every barrier below is met by all waves.
          const bool sliceb = wsub != 0;
          float* hs = sliceb ? h2 : h1;
          const float* a = hs + r * SH + q * 4;
          {
            f32x4 acc2[NTI1];
#pragma unroll
            for (int t = 0; t < NTI1; ++t) acc2[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            t0 = L2HMC_CYCLES_NOW();
            stream_layer<NTI1, Cfg::KC2, DP2P, NTI1, 1>(
                R2P, wp2, [&](int kc) { return *reinterpret_cast<const f32x4*>(a + kc * 16); }, acc2, !sliceb, 0);
            ring_prime<3 * NTIH, DPHP, 3 * NTIH, 1>(R3P, wph, !sliceb, Cfg::KC2, 0);
            L2HMC_CYCLES_ADD(ft, 1, t0);
            {
              [[maybe_unused]] const unsigned long long tb = L2HMC_CYCLES_NOW();
              __syncthreads();                    // every wave has read its slice's rows: they take layer 2's output
              L2HMC_CYCLES_ADD(ft, 6, tb);
            }
            t0 = L2HMC_CYCLES_NOW();
#pragma unroll
            for (int t = 0; t < NTI1; ++t) {
              const int c0 = (wimg * NTI1 + t) * 16 + q * 4;
              const f32x4 b = *reinterpret_cast<const f32x4*>(cn + 3 * H + c0);
              f32x4 hv;
#pragma unroll
              for (int e = 0; e < 4; ++e) hv[e] = relu_nan(acc2[t][e] + b[e]);
              *reinterpret_cast<f32x4*>(hs + r * SH + c0) = hv;
            }
            L2HMC_CYCLES_ADD(ft, 4, t0);
          }
          {
            [[maybe_unused]] const unsigned long long tb = L2HMC_CYCLES_NOW();
            __syncthreads();
            L2HMC_CYCLES_ADD(ft, 6, tb);
          }
          f32x4 acch[3 * NTIH];
#pragma unroll
          for (int t = 0; t < 3 * NTIH; ++t) acch[t] = f32x4{0.f, 0.f, 0.f, 0.f};
          t0 = L2HMC_CYCLES_NOW();
          stream_layer<3 * NTIH, Cfg::KC2, DPHP, 3 * NTIH, 1>(
              R3P, wph, [&](int kc) { return *reinterpret_cast<const f32x4*>(a + kc * 16); }, acch, !sliceb, 0);
          L2HMC_CYCLES_ADD(ft, 2, t0);
          t0 = L2HMC_CYCLES_NOW();
          const float* bhd = cn + 4 * H;
          const float* es = bhd + 3 * D;
          const float* eq = es + D;
          const int d = dirl;
          f32x4 S[NTIH], Tt[NTIH], Q[NTIH];
#pragma unroll
          for (int t = 0; t < NTIH; ++t) {
            const int c0 = wimg * (D / IMGW) + t * 16 + q * 4;      // row r, columns c0 .. c0 + 3
            const f32x4 b_s = *reinterpret_cast<const f32x4*>(bhd + c0);
            const f32x4 b_t = *reinterpret_cast<const f32x4*>(bhd + D + c0);
            const f32x4 b_q = *reinterpret_cast<const f32x4*>(bhd + 2 * D + c0);
            const f32x4 e_s = *reinterpret_cast<const f32x4*>(es + c0);
            const f32x4 e_q = *reinterpret_cast<const f32x4*>(eq + c0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              float s_, t_, q_;
              heads_stq(acch[0 * NTIH + t][e], acch[1 * NTIH + t][e], acch[2 * NTIH + t][e], b_s[e], b_t[e], b_q[e], e_s[e],
                        e_q[e], net.q_tanh, s_, t_, q_);
              S[t][e] = s_; Tt[t][e] = t_; Q[t][e] = q_;
            }
          }
          // the slice's kick on its section's columns and row r's log-det share, one chain of adds per lane over both
          // tiles, then the cross-lane steps: the order of the 4-wave forms
          auto kick_slice = [&]() {
            float ld = 0.f;
#pragma unroll
            for (int t = 0; t < NTIH; ++t) {
              const int idx = r * SX + wimg * (D / IMGW) + t * 16 + q * 4;
              const f32x4 g = *reinterpret_cast<const f32x4*>(gs + idx);
              const f32x4 v = *reinterpret_cast<const f32x4*>(vs + idx);
              f32x4 vn;
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                float s;
                vn[e] = lf_kick<ExpFast>(v[e], g[e], S[t][e], Tt[t][e], Q[t][e], eps, d, s);
                ld += s;
              }
              *reinterpret_cast<f32x4*>(vs + idx) = vn;
            }
            ld += __shfl_xor(ld, 16, 64);
            ld += __shfl_xor(ld, 32, 64);
            if (q == 0) ldw[wimg * kFM + r] += ld;
          };
          if (!sliceb) kick_slice();
          L2HMC_CYCLES_ADD(ft, 5, t0);
          {
            [[maybe_unused]] const unsigned long long tb = L2HMC_CYCLES_NOW();
            __syncthreads();                      // slice A's v' and log-det sums are in place
            L2HMC_CYCLES_ADD(ft, 6, tb);
          }
          t0 = L2HMC_CYCLES_NOW();
          if (sliceb) {
            kick_slice();
            // the next net call is the next step's first position sub-update: its second input is keep (.) x, under the
            // masks of that step (in skm / scp / sel since the barrier behind layer 1)
            const bool l1n = ACTOK && SPLIT && p.l1_img && p.heads_img && __builtin_amdgcn_readfirstlane(sel[0] & sel[1]) != 0;
#pragma unroll
            for (int t = 0; t < NTIH; ++t) {
              const int c0 = wimg * (D / IMGW) + t * 16 + q * 4;
              const int idx = r * SX + c0;
              const f32x4 mf = *reinterpret_cast<const f32x4*>(skm + c0);
              const f32x4 mb = *reinterpret_cast<const f32x4*>(skm + D + c0);
              const f32x4 x = *reinterpret_cast<const f32x4*>(xs + idx);
              f32x4 kx;
#pragma unroll
              for (int e = 0; e < 4; ++e) kx[e] = keep_of(mf[e], mb[e], d, 0) * x[e];
              if (l1n) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                  if (keep_of(mf[e], mb[e], d, 0) != 0.f) stg[r * SX + scp[c0 + e]] = kx[e];
                  else if (kx[e] != kx[e]) spz[r] = kx[e];
                }
              } else {
                *reinterpret_cast<f32x4*>(gs + idx) = kx;
              }
            }
          }
          L2HMC_CYCLES_ADD(ft, 5, t0);
          {
            [[maybe_unused]] const unsigned long long tb = L2HMC_CYCLES_NOW();
            __syncthreads();
            L2HMC_CYCLES_ADD(ft, 6, tb);
          }
          return;
        }
      }
      ring_prime<NT1, DP2, NTI1>(R2, wp2, zig, Cfg::KC2, to1);      // layer-2 weights start flowing under the epilogue + barrier
      L2HMC_CYCLES_ADD(ft, 0, t0);
      t0 = L2HMC_CYCLES_NOW();
      [[maybe_unused]] unsigned gmask = 0;
#pragma unroll
      for (int t = 0; t < NT1; ++t) {
        const int c0 = (wave * NT1 + t) * 16 + q * 4;          // this lane: row r, columns c0 .. c0 + 3
        const f32x4 b = *reinterpret_cast<const f32x4*>(cn + c0);
        const f32x4 w0 = *reinterpret_cast<const f32x4*>(cn + H + c0);
        const f32x4 w1 = *reinterpret_cast<const f32x4*>(cn + 2 * H + c0);
        f32x4 hv;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          hv[e] = relu_nan(acc[t][e] + b[e] + (tcr * w0[e] + tsr * w1[e]));
          if constexpr (TAPE) gmask |= (hv[e] > 0.f ? 1u : 0u) << (t * 4 + e);
        }
        *reinterpret_cast<f32x4*>(h1 + r * SH + c0) = hv;
      }
      if constexpr (TAPE) {
        // one 32-bit word per lane of the 4-wave image wave (the reverse kernel's layout); two waves of a section write its halves
        const size_t word = ((size_t)(callidx * 2 + 0) * gridDim.x + blockIdx.x) * (64 * IMGW) + wimg * 64 + lane;
        if constexpr (RW == 1) tp.gate[word] = gmask;
        else reinterpret_cast<unsigned short*>(tp.gate)[word * 2 + wsub] = (unsigned short)gmask;
      }
      L2HMC_CYCLES_ADD(ft, 3, t0);
    }
    {
      [[maybe_unused]] const unsigned long long tb = L2HMC_CYCLES_NOW();
      __syncthreads();
      L2HMC_CYCLES_ADD(ft, 6, tb);
    }
    if constexpr (TAPE) tape_rows(tp.h1, h1);
    // ----- layer 2
    {
      f32x4 acc[NT1];
#pragma unroll
      for (int t = 0; t < NT1; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      const float* a = h1 + r * SH + q * 4;
      [[maybe_unused]] unsigned long long t0 = L2HMC_CYCLES_NOW();
      stream_layer<NT1, Cfg::KC2, DP2, NTI1>(
          R2, wp2, [&](int kc) { return *reinterpret_cast<const f32x4*>(a + kc * 16); }, acc, zig, to1);
      if (ACTOK && actv) {
        if (wv < 4) ring_prime<3 * NTH, DPH, 3, 1>(R3, wpa, zig, Cfg::KC2, 0);
      } else {
        ring_prime<3 * NTH, DPH, 3 * NTIH, TSH>(R3, wph, zig, Cfg::KC2, toh);
      }
      L2HMC_CYCLES_ADD(ft, 1, t0);
      t0 = L2HMC_CYCLES_NOW();
      [[maybe_unused]] unsigned gmask = 0;
#pragma unroll
      for (int t = 0; t < NT1; ++t) {
        const int c0 = (wave * NT1 + t) * 16 + q * 4;
        const f32x4 b = *reinterpret_cast<const f32x4*>(cn + 3 * H + c0);
        f32x4 hv;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          hv[e] = relu_nan(acc[t][e] + b[e]);
          if constexpr (TAPE) gmask |= (hv[e] > 0.f ? 1u : 0u) << (t * 4 + e);
        }
        *reinterpret_cast<f32x4*>(h2 + r * SH + c0) = hv;
      }
      if constexpr (TAPE) {
        // one 32-bit word per lane of the 4-wave image wave (the reverse kernel's layout); two waves of a section write its halves
        const size_t word = ((size_t)(callidx * 2 + 1) * gridDim.x + blockIdx.x) * (64 * IMGW) + wimg * 64 + lane;
        if constexpr (RW == 1) tp.gate[word] = gmask;
        else reinterpret_cast<unsigned short*>(tp.gate)[word * 2 + wsub] = (unsigned short)gmask;
      }
      L2HMC_CYCLES_ADD(ft, 4, t0);
    }
    {
      [[maybe_unused]] const unsigned long long tb = L2HMC_CYCLES_NOW();
      __syncthreads();
      L2HMC_CYCLES_ADD(ft, 6, tb);
    }
    if constexpr (TAPE) tape_rows(tp.h2, h2);
    // ----- heads + update
    {
      f32x4 acc[3 * NTH];
#pragma unroll
      for (int t = 0; t < 3 * NTH; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      const float* a = h2 + r * SH + q * 4;
      [[maybe_unused]] unsigned long long t0 = L2HMC_CYCLES_NOW();
      if (ACTOK && actv) {
        if (wv < 4)
          stream_layer<3 * NTH, Cfg::KC2, DPH, 3, 1>(
              R3, wpa, [&](int kc) { return *reinterpret_cast<const f32x4*>(a + kc * 16); }, acc, zig, 0);
      } else {
        stream_layer<3 * NTH, Cfg::KC2, DPH, 3 * NTIH, TSH>(
            R3, wph, [&](int kc) { return *reinterpret_cast<const f32x4*>(a + kc * 16); }, acc, zig, toh);
      }
      L2HMC_CYCLES_ADD(ft, 2, t0);
      t0 = L2HMC_CYCLES_NOW();
      float ld = 0.f;                       // this lane's share of row r's log-det
      const float* bhd = cn + 4 * H;
      const float* es = bhd + 3 * D;
      const float* eq = es + D;
      const int d = dirl;
      if (ACTOK && actv) {
        // lane (q, r) of wave w < 4: row r, active columns al[16 w + 4 q + e]; wave w >= 4: kept columns il[...]
        const int* al = scol + asense * (D / 2);
        const int* il = scol + (asense ^ 1) * (D / 2);
        if (wv < 4) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int c = al[wv * 16 + q * 4 + e];
            const int idx = r * SX + c;
            float S, Tt, Q, s, omk;
            heads_stq(acc[0][e], acc[1][e], acc[2][e], bhd[c], bhd[D + c], bhd[2 * D + c], es[c], eq[c], net.q_tanh, S,
                      Tt, Q);
            const float xn = lf_drift<ExpFast>(xs[idx], vs[idx], keep_of(skm[c], skm[D + c], d, sub), S, Tt, Q, eps, d, s,
                                               omk);
            xs[idx] = xn;
            stg[idx] = omk * s;
            // (the columns this sub-update moves are the ones the next one keeps)
            if (prep_next_mask) gs[l1c ? r * SX + scp[c] : idx] = omk * xn;
          }
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int c = il[(wv - 4) * 16 + q * 4 + e];
            const int idx = r * SX + c;
            stg[idx] = 0.f;
            if (prep_next_mask) {
              const float kx = (1.f - keep_of(skm[c], skm[D + c], d, sub)) * xs[idx];
              if (!l1c) gs[idx] = kx;
              else if (kx != kx) spz[kFM + r] = kx;
            }
          }
          if (l1c && wv == 4 && q == 0) spz[sub * kFM + r] = 0.f;      // this call's poison is spent
        }
      } else {
#pragma unroll
      for (int t = 0; t < NTH; ++t) {
        const int c0 = wave * (D / kFWaves) + t * 16 + q * 4;      // row r, columns c0 .. c0 + 3
        const f32x4 b_s = *reinterpret_cast<const f32x4*>(bhd + c0);
        const f32x4 b_t = *reinterpret_cast<const f32x4*>(bhd + D + c0);
        const f32x4 b_q = *reinterpret_cast<const f32x4*>(bhd + 2 * D + c0);
        const f32x4 e_s = *reinterpret_cast<const f32x4*>(es + c0);
        const f32x4 e_q = *reinterpret_cast<const f32x4*>(eq + c0);
        const f32x4 mf = *reinterpret_cast<const f32x4*>(skm + c0);
        const f32x4 mb = *reinterpret_cast<const f32x4*>(skm + D + c0);
        const int idx = r * SX + c0;
        f32x4 S, Tt, Q;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float s_, t_, q_;
          heads_stq(acc[0 * NTH + t][e], acc[1 * NTH + t][e], acc[2 * NTH + t][e], b_s[e], b_t[e], b_q[e], e_s[e], e_q[e],
                    net.q_tanh, s_, t_, q_);
          S[e] = s_; Tt[e] = t_; Q[e] = q_;
        }
        if constexpr (TAPE) {
          if (r < nrow) {
            const size_t plane = (size_t)p.rows * D;
            float* o = tp.stq + (size_t)callidx * 3 * plane + ((size_t)row0 + r) * D + c0;
            tape_store(o, S);
            tape_store(o + plane, Tt);
            tape_store(o + 2 * plane, Q);
          }
        }
        if (mode == 1) {
          // gauge_dynamics.py:497-506 (fwd), :549-559 (bwd)
          const f32x4 g = *reinterpret_cast<const f32x4*>(gs + idx);
          const f32x4 v = *reinterpret_cast<const f32x4*>(vs + idx);
          f32x4 vn;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float s;
            vn[e] = lf_kick<ExpFast>(v[e], g[e], S[e], Tt[e], Q[e], eps, d, s);
            ld += s;
            if constexpr (RW > 1) { ld_k[e] = 1.f; ld_s[e] = s; }
          }
          *reinterpret_cast<f32x4*>(vs + idx) = vn;
          // the next net call is the first position sub-update: its second input is keep (.) x
          if (prep_next_mask) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(xs + idx);
            f32x4 kx;
#pragma unroll
            for (int e = 0; e < 4; ++e) kx[e] = keep_of(mf[e], mb[e], d, 0) * x[e];
            if (l1c) {
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                if (keep_of(mf[e], mb[e], d, 0) != 0.f) stg[r * SX + scp[c0 + e]] = kx[e];
                else if (kx[e] != kx[e]) spz[r] = kx[e];
              }
            } else {
              *reinterpret_cast<f32x4*>(gs + idx) = kx;
            }
          }
        } else {
          // gauge_dynamics.py:519-531 (fwd), :574-584 (bwd); keep mask per direction and sub-update
          const f32x4 x = *reinterpret_cast<const f32x4*>(xs + idx);
          const f32x4 v = *reinterpret_cast<const f32x4*>(vs + idx);
          f32x4 xn, kx;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float s, omk;
            xn[e] = lf_drift<ExpFast>(x[e], v[e], keep_of(mf[e], mb[e], d, sub), S[e], Tt[e], Q[e], eps, d, s, omk);
            ld += omk * s;
            if constexpr (RW > 1) { ld_k[e] = omk; ld_s[e] = s; }
            kx[e] = omk * xn[e];
          }
          *reinterpret_cast<f32x4*>(xs + idx) = xn;
          // second sub-update follows: its keep mask is the complement (gauge_dynamics.py:434-437, :472-475)
          if (prep_next_mask) *reinterpret_cast<f32x4*>(gs + idx) = kx;
        }
      }
      // row r's log-det share of this wave: lanes r, r + 16, r + 32, r + 48 (fixed order: bit-reproducible)
      if constexpr (RW == 1) {
        ld += __shfl_xor(ld, 16, 64);
        ld += __shfl_xor(ld, 32, 64);
        if (q == 0) ldw[wave * kFM + r] += ld;
      } else {
        // Two waves share an image wave's columns.  The bits of the 4-wave forms are those of ONE chain of adds per
        // lane over both waves' tiles, then the cross-lane steps: the even wave hands its lane sum over, the odd wave
        // continues the chain with its own four terms behind the barrier below (ld_k, ld_s) and does the rest.
        if (wsub == 0) ldx[wimg * 64 + lane] = ld;
      }
      }
      L2HMC_CYCLES_ADD(ft, 5, t0);
    }
    {
      [[maybe_unused]] const unsigned long long tb = L2HMC_CYCLES_NOW();
      __syncthreads();
      L2HMC_CYCLES_ADD(ft, 6, tb);
    }
    if (ACTOK && actv) {
      // the chain of adds of the all-columns form over both waves' columns of the section; a kept column adds +-0
      if (wsub == 1) {
        float ld = 0.f;
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int e = 0; e < 4; ++e) ld += stg[r * SX + (2 * wimg + h) * 16 + q * 4 + e];
        ld += __shfl_xor(ld, 16, 64);
        ld += __shfl_xor(ld, 32, 64);
        if (q == 0) ldw[wimg * kFM + r] += ld;
      }
    } else if constexpr (RW > 1) {
      if (wsub == 1) {
        float ld = ldx[wimg * 64 + lane];
#pragma unroll
        for (int e = 0; e < 4; ++e) ld += ld_k[e] * ld_s[e];      // (the same contracted multiply-add as the chain above)
        ld += __shfl_xor(ld, 16, 64);
        ld += __shfl_xor(ld, 32, 64);
        if (q == 0) ldw[wimg * kFM + r] += ld;
      }
    }
  };

  // ---- leapfrog steps -----------------------------------------------------------
  const float two_pi = 6.28318530717958647692f;
  // time encoding of this lane's row at a step (gauge_dynamics.py:453-457)
  auto step_time = [&](int step, float& tc, float& ts) {
    const int sf = step, sb = p.num_steps - 1 - step;
    const float af = two_pi * (float)sf / (float)p.num_steps, ab = two_pi * (float)sb / (float)p.num_steps;
    const float tcf = cosf(af), tsf = sinf(af), tcb = cosf(ab), tsb = sinf(ab);
    tc = dirl ? tcb : tcf;
    ts = dirl ? tsb : tsf;
  };
  // masks, column lists and compact-k map of a step -> LDS (the caller puts a barrier in front of their readers)
  auto load_step_masks = [&](int step) {
    const int sf = step, sb = p.num_steps - 1 - step;
    for (int i = tid; i < D; i += kFThreads) {
      skm[i] = p.masks[(size_t)sf * D + i];
      skm[D + i] = p.masks[(size_t)sb * D + i];
    }
    if (ACTOK && SPLIT && p.heads_meta) {
      arow = sdw ? sb : sf;
      for (int i = tid; i < D; i += kFThreads) scol[i] = p.heads_meta[2 * p.num_steps + arow * D + i];
      if (tid < 2) sel[tid] = p.heads_meta[arow * 2 + tid];
      if (p.l1_img)
        for (int i = tid; i < D; i += kFThreads) scp[i] = p.heads_meta[2 * p.num_steps + (p.num_steps + arow) * D + i];
    }
  };
  const bool PAIR = PAIROK && !p.single_kicks;
  bool paired_in = false;              // this step's first half-kick ran inside the previous step's paired call
  for (int step = p.step_begin; step < p.step_end; ++step) {
    float tcr, tsr, tcr2 = 0.f, tsr2 = 0.f;
    step_time(step, tcr, tsr);
    const bool pair_out = PAIR && step + 1 < p.step_end;
    if (!paired_in) {
      load_step_masks(step);
      // (gs holds the force of the current x: from the prologue or the previous step's last kick)
      __syncthreads();
    }
    // the four network calls of a leapfrog step run through ONE copy of the code (runtime parameters,
    // wave-uniform branches): the kernel stays well inside the instruction cache
#pragma nounroll
    for (int call = paired_in ? 1 : 0; call < 4; ++call) {
      const bool is_v = call == 0 || call == 3;
      const bool pair = pair_out && call == 3;
      if (call == 3) {
        [[maybe_unused]] const unsigned long long tf = L2HMC_CYCLES_NOW();
        float unused[1];
        force_pass<kFM, kTPC, 1, D, SX, SP, LADDER>(cl, xs, sp, gs, unused);   // force at the new position
        L2HMC_CYCLES_ADD(ft, 7, tf);
        // paired call: no call of this step reads a mask any more (call 3 uses none), so the next step's take their
        // place now; the barrier behind the first layer stands between these writes and slice B's reads
        if (pair) {
          load_step_masks(step + 1);
          step_time(step + 1, tcr2, tsr2);
        }
      }
      // call 0: momentum half-kick (+ keep (.) x into gs)      call 1: position sub-update 1 (+ complement mask)
      // call 2: position sub-update 2                          call 3: second momentum half-kick (product kept),
      //                                                                paired with the next step's call 0 if there is one
      const int l1 = call == 0 ? (keep_v_valid ? 2 : 0) : call == 1 ? 3 : call == 2 ? 4 : 1;
      net_update(is_v ? p.vnet : p.xnet, is_v ? cv : cx, is_v ? xs : vs, is_v ? 1 : 2, call == 2 ? 1 : 0,
                 call < 2, l1, is_v, tcr, tsr, 2 * step + (call == 0 || call == 1 ? 0 : 1), pair, tcr2, tsr2);
    }
    keep_v_valid = true;
    paired_in = pair_out;
  }

  // ---- epilogue: energies, accept probability, write back -------------------------
  float act1[1], kin1[1];
  force_pass<kFM, kTPC, 1, D, SX, SP, LADDER>(cl, xs, sp, gs, act1);
  kinetic_pass<kFM, kTPC, 1, D, SX>(cl, vs, kin1);
  if (STEPM) {
    step_accept_probs<kFM, 1, IMGW, LADDER>(cl, ldw, act0, act1, kin0, kin1, spx);
    __syncthreads();
    // forward / backward rows of chain k (x, v: row stride SX) and their accept probabilities
    const float* xfr = xs;
    const float* xbr = xs + (kFM / 2) * SX;
    const float* vfr = vs;
    const float* vbr = vs + (kFM / 2) * SX;
    const float* pfr = spx;
    const float* pbr = spx + kFM / 2;
    if (SPLIT) {
      // ---- hand-off between the two workgroups of a pair (cdna_hip_programming.md, Guideline 16, counter form):
      //      both publish their rows, the one that draws ticket 1 takes its partner's and finishes the 16 chains.
      //      Nobody waits: the first to arrive simply ends.
      constexpr int HW = 2 * kFM * D + kFM;           // floats per workgroup in step_hand
      float* mine = p.step_hand + (size_t)blockIdx.x * HW;
      for (int i = tid; i < kFM * (D / 4); i += kFThreads) {
        const int rr = i / (D / 4), c4 = (i - rr * (D / 4)) * 4;
        *reinterpret_cast<f32x4*>(mine + rr * D + c4) = *reinterpret_cast<const f32x4*>(xs + rr * SX + c4);
        if (p.step_vprop)
          *reinterpret_cast<f32x4*>(mine + (kFM + rr) * D + c4) = *reinterpret_cast<const f32x4*>(vs + rr * SX + c4);
      }
      if (tid < kFM) mine[2 * kFM * D + tid] = spx[tid];
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      int* is_last = sdir;                              // (sdir is free: every lane holds its row's direction)
      __syncthreads();
      if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int got = __hip_atomic_fetch_add(p.step_ticket + (blockIdx.x >> 1), 1, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
        if (got == 1) {
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          // nobody takes this ticket again in this launch: it is left at 0, as the step sums' ticket is (the clear
          // kernel ahead of the launch stays: a workspace holds anything on entry)
          __hip_atomic_store(p.step_ticket + (blockIdx.x >> 1), 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        is_last[0] = got == 1;
      }
      __syncthreads();
      if (!is_last[0]) return;
      // the partner's rows -> h2 (free): x [16][SX], v [16][SX], p [16]
      const float* other = p.step_hand + (size_t)(blockIdx.x ^ 1u) * HW;
      float* ox = h2;
      float* ov = h2 + kFM * SX;
      float* op = h2 + 2 * kFM * SX;
      for (int i = tid; i < kFM * (D / 4); i += kFThreads) {
        const int rr = i / (D / 4), c4 = (i - rr * (D / 4)) * 4;
        *reinterpret_cast<f32x4*>(ox + rr * SX + c4) = *reinterpret_cast<const f32x4*>(other + rr * D + c4);
        if (p.step_vprop)
          *reinterpret_cast<f32x4*>(ov + rr * SX + c4) = *reinterpret_cast<const f32x4*>(other + (kFM + rr) * D + c4);
      }
      if (tid < kFM) op[tid] = other[2 * kFM * D + tid];
      __syncthreads();
      if (sdw == 0) {
        xbr = ox; vbr = ov; pbr = op;
      } else {
        xfr = ox; vfr = ov; pfr = op;
        xbr = xs; vbr = vs; pbr = spx;
      }
    }
    // ---- mix, accept, measure, sum, wrap (fused_step.h); x_in -> gs rows, x_out -> h1 rows (both free now)
    float* gin = gs;
    float* gout = h1;
    step_mix_accept<kFThreads, D, SX>(p, wg, xfr, xbr, vfr, vbr, pfr, pbr, gin, gout);
    step_observables<kFM, kTPC, 1, D, SX>(p, wg, cl, gin, gout);
    // (SPLIT: a pair leaves the partial sums of the two 8-chain groups the paired layout gives its workgroups --
    //  the same entries, the same order; only the pairs' last arrivers take part)
    const int ngrp = SPLIT ? 2 : 1;
    const int64_t slot0 = SPLIT ? (int64_t)(blockIdx.x >> 1) * 2 : (int64_t)blockIdx.x;
    const int nfin = SPLIT ? (int)(gridDim.x >> 1) : (int)gridDim.x;
    const int npart = SPLIT ? (int)((p.step_Bl + kFM / 2 - 1) / (kFM / 2)) : (int)gridDim.x;
    step_sums<kFThreads, kFThreads>(p, wg, ngrp, slot0, npart, nfin, /*fin=*/vs);     // (vs is dead)
    step_write_next<kFThreads, D, SX>(p, wg, gout);
    return;
  }
  traj_logdet_accept<kFM, 1, IMGW, TAPE && LADDER>(p, wg, cl, ldw, act0, act1, kin0, kin1);
#ifdef L2HMC_STAMPS
  if (p.stamps && tid == 0) {
    unsigned long long rt1;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rt1)::"memory");
    ft[9] = L2HMC_CYCLES_NOW() - ft_start;
    for (int i = 0; i < 10; ++i) p.stamps[blockIdx.x * 12 + i] = ft[i];
    p.stamps[blockIdx.x * 12 + 10] = rt0;
    p.stamps[blockIdx.x * 12 + 11] = rt1;
  }
#endif
  traj_write_back<kFM, kFThreads, D, SX>(p, wg, xs, vs);
}

// the split form's pair tickets -> 0, launched on the step's stream right ahead of the split kernel
__global__ __launch_bounds__(256) void clear_tickets_kernel(int* __restrict__ tickets, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) tickets[i] = 0;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// l2hmc_gauge_pack_heads image: int eligibility [N][2], int columns [N][2][D / 2], int compact first-layer k [N][D],
// then (256-byte aligned) the heads sections and, behind them, the kept-column first-layer sections
static size_t heads_meta_bytes(int N, int D) { return align_up(sizeof(int) * ((size_t)2 * N + (size_t)2 * N * D), 256); }
static size_t heads_sections_bytes(int N, int D, int H) { return sizeof(float) * (size_t)2 * N * 3 * (D / 2) * H; }
static size_t l1_sections_bytes(int N, int D, int H) { return sizeof(float) * (size_t)2 * N * (D / 2) * H; }
// shapes with a whole-trajectory kernel: GenericNet on D=128 (H=512), and the dense trunk of ConvNet3D on the
// 8x8 lattice (features 64+64, H=256)
static int fused_generic_net(const l2hmc_dense_net* n) {
  return n->D == 128 && n->H == 512 && n->Ka == 128 && n->Kb == 128;
}
static int fused_conv_net(const l2hmc_dense_net* n) {
  return n->D == 128 && n->H == 256 && n->Ka == 64 && n->Kb == 64;
}
// ... and the two GenericNet shapes of a torus-exact plan on D = 128 (fused_traj_ncp.hip; K1 = 3 D)
int fused_net_supported(const l2hmc_dense_net* n) {
  return fused_generic_net(n) || fused_conv_net(n) || fused_ncp_net_supported(n);
}

// L2HMC_PLAN_TILES16_ONLY keeps every batch on the 16-row form (A/B and the bit-identity test)
static bool subtile_enabled(const l2hmc_gauge_plan* p) { return !(p->flags & L2HMC_PLAN_TILES16_ONLY); }
// CUs of the current device (one 16-row workgroup each per round); asked once per device
static int device_cu_count() {
  static std::atomic<int> cached[16];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return 256;
  int n = cached[dev].load(std::memory_order_relaxed);
  if (n <= 0) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cached[dev].store(n, std::memory_order_relaxed);
  }
  return n;
}
int fused_plan_supported(const l2hmc_gauge_plan* p) {
  if (p->hmc || !p->xnet.packed || !p->vnet.packed || 2 * p->T * p->X != 128 || (p->X & (p->X - 1)) != 0) return 0;
  // the torus-exact mode runs layer by layer (leapfrog.hip) unless the plan asks for its whole-step kernel and has it
  if (p->flags & L2HMC_PLAN_PERIODIC) return fused_ncp_plan(p);
  if (p->flags & L2HMC_PLAN_CONV3D)
    return fused_conv_net(&p->xnet) && fused_conv_net(&p->vnet) && p->T == 8 && p->X == 8 && p->xfront.F == 8 &&
           p->vfront.F == 8;
  return fused_generic_net(&p->xnet) && fused_generic_net(&p->vnet);
}

int launch_fused_trajectory(const l2hmc_gauge_plan* p, float beta, int step_begin, int step_end,
                            const float* x0, const float* v0, const int* dir, int64_t rows, float* x_out,
                            float* v_out, float* logdet, int logdet_accumulate, float* p_accept,
                            hipStream_t stream, int64_t x_mod, int64_t dir_split, const FusedTape* tape_x,
                            const FusedTape* tape_v, const float* betas, int64_t beta_mod, int64_t beta_stride) {
  // (a taped launch: the training forward of a plan with L2HMC_PLAN_PERIODIC_TAPE, whether or not it samples in one launch)
  const bool ncp_tape = tape_x && tape_v && fused_ncp_tape_plan(p);
  if (fused_ncp_plan(p) || ncp_tape) {
    // torus-exact plans: their own kernel, one form for every batch (fused_traj_ncp.hip), ahead of any form selection
    L2HMC_REQUIRE(ncp_tape || (!tape_x && !tape_v && !betas),
                  "fused trajectory: a periodic plan has a taped or per-row-beta form with L2HMC_PLAN_PERIODIC_TAPE only");
    FusedArgs a{};
    if (ncp_tape) {
      a.tx = *tape_x;
      a.tv = *tape_v;
      a.step_betas = betas; a.step_beta_mod = beta_mod; a.step_beta_stride = beta_stride;
    }
    a.T = p->T; a.X = p->X; a.num_steps = p->num_steps; a.step_begin = step_begin; a.step_end = step_end;
    a.eps = p->eps; a.beta = beta; a.masks = p->masks; a.xnet = p->xnet; a.vnet = p->vnet;
    a.x0 = x0; a.v0 = v0; a.dir = dir; a.rows = rows; a.x_out = x_out; a.v_out = v_out;
    a.x_mod = x_mod; a.dir_split = dir_split;
    a.logdet = logdet; a.logdet_accumulate = logdet_accumulate; a.p_accept = p_accept;
    return launch_fused_ncp(a, (p->flags & L2HMC_PLAN_RECOMPUTE) != 0, stream);
  }
  const bool conv = (p->flags & L2HMC_PLAN_CONV3D) != 0;
  using CfgG = FusedCfg<128, 512, 128, false>;
  using CfgC = FusedCfg<128, 256, 64, true>;
  static DeviceOnce attr_once;
  const bool tape = tape_x && tape_v;
  const size_t lds = sizeof(float) * (conv ? CfgC::LDS_FLOATS : CfgG::LDS_FLOATS);
  if (attr_once.pending()) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&gauge_traj_fused_kernel<128, 512, 128, false>),
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(sizeof(float) * CfgG::LDS_FLOATS)) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void*>(&gauge_traj_fused_kernel<128, 256, 64, true>),
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(sizeof(float) * CfgC::LDS_FLOATS)) != hipSuccess) {
      set_error("fused trajectory: cannot reserve %zu B of LDS", lds);
      return L2HMC_ERR_HIP;
    }
    attr_once.done();
  }
  FusedArgs a{};
  a.T = p->T; a.X = p->X; a.num_steps = p->num_steps; a.step_begin = step_begin; a.step_end = step_end;
  a.eps = p->eps; a.beta = beta; a.masks = p->masks; a.xnet = p->xnet; a.vnet = p->vnet;
  a.xfront = p->xfront; a.vfront = p->vfront;
  a.x0 = x0; a.v0 = v0; a.dir = dir; a.rows = rows; a.x_out = x_out; a.v_out = v_out;
  a.x_mod = x_mod; a.dir_split = dir_split;
  a.logdet = logdet; a.logdet_accumulate = logdet_accumulate; a.p_accept = p_accept;
  a.single_kicks = (p->flags & L2HMC_PLAN_SINGLE_KICKS) != 0;
  if (tape) {
    L2HMC_REQUIRE(step_begin == 0, "fused trajectory: taping needs the whole trajectory");
    L2HMC_REQUIRE(!conv || (tape_x->feat && tape_v->feat), "fused trajectory: ConvNet3D taping needs the feature tape");
    L2HMC_REQUIRE(tape_x->in && tape_x->h1 && tape_x->h2 && tape_x->stq && tape_x->st && tape_v->in && tape_v->h1 &&
                      tape_v->h2 && tape_v->stq && tape_v->st && tape_x->gate && tape_v->gate,
                  "fused trajectory: NULL tape pointer");
    a.tx = *tape_x;
    a.tv = *tape_v;
    static DeviceOnce tape_once;
    if (tape_once.pending()) {
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(&gauge_traj_fused_kernel<128, 512, 128, false, true>),
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(sizeof(float) * CfgG::LDS_FLOATS)) != hipSuccess ||
          hipFuncSetAttribute(reinterpret_cast<const void*>(&gauge_traj_fused_kernel<128, 256, 64, true, true>),
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(sizeof(float) * CfgC::LDS_FLOATS)) != hipSuccess) {
        set_error("fused trajectory: cannot reserve %zu B of LDS", lds);
        return L2HMC_ERR_HIP;
      }
      tape_once.done();
    }
  }
  if (betas) {
    // a ladder: the taped instances that read a beta per row (FusedArgs::step_beta_mod); `beta` is what a dead row takes
    L2HMC_REQUIRE(tape && beta_mod > 0 && (beta_stride == 0 || beta_stride == 1),
                  "fused trajectory: a beta per row needs the tape, a modulus > 0 and an element stride of 0 or 1");
    a.step_betas = betas; a.step_beta_mod = beta_mod; a.step_beta_stride = beta_stride;
    static DeviceOnce ladder_once;
    if (ladder_once.pending()) {
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(&gauge_traj_fused_kernel<128, 512, 128, false, true, true>),
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(sizeof(float) * CfgG::LDS_FLOATS)) != hipSuccess ||
          hipFuncSetAttribute(reinterpret_cast<const void*>(&gauge_traj_fused_kernel<128, 256, 64, true, true, true>),
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(sizeof(float) * CfgC::LDS_FLOATS)) != hipSuccess) {
        set_error("fused trajectory: cannot reserve %zu B of LDS", lds);
        return L2HMC_ERR_HIP;
      }
      ladder_once.done();
    }
  }
#ifdef L2HMC_STAMPS
  a.stamps = g_stamp_cls == 5 ? g_stamp_buf : nullptr;
  a.stagger = g_fused_stagger;
#endif
  // batches that cannot put a 16-row tile on every CU: the sub-tile form (4 or 8 rows per workgroup, same bits)
  if (!conv && !tape && subtile_enabled(p)) {
    if (const int rpw = fused4_rows_per_wg(rows, device_cu_count())) return launch_fused4(a, rpw, stream);
    // more than one round of 16-row workgroups: the 32-row form (each weight fragment feeds two MFMAs)
    if (rows > (int64_t)kFM * device_cu_count()) return launch_fused32(a, stream);
  }
  const dim3 grid((unsigned)ceil_div(rows, kFM));
  prof_before(kProfFused, stream);
  if (conv && betas)
    hipLaunchKernelGGL((gauge_traj_fused_kernel<128, 256, 64, true, true, true>), grid, dim3(CfgC::THREADS), lds, stream,
                       a);
  else if (betas)
    hipLaunchKernelGGL((gauge_traj_fused_kernel<128, 512, 128, false, true, true>), grid, dim3(CfgG::THREADS), lds,
                       stream, a);
  else if (conv && tape)
    hipLaunchKernelGGL((gauge_traj_fused_kernel<128, 256, 64, true, true>), grid, dim3(CfgC::THREADS), lds, stream, a);
  else if (conv)
    hipLaunchKernelGGL((gauge_traj_fused_kernel<128, 256, 64, true>), grid, dim3(CfgC::THREADS), lds, stream, a);
  else if (tape)
    hipLaunchKernelGGL((gauge_traj_fused_kernel<128, 512, 128, false, true>), grid, dim3(CfgG::THREADS), lds, stream, a);
  else
    hipLaunchKernelGGL((gauge_traj_fused_kernel<128, 512, 128, false>), grid, dim3(CfgG::THREADS), lds, stream, a);
  prof_after(kProfFused, stream);
  L2HMC_CHECK_LAUNCH("gauge_traj_fused");
  return L2HMC_OK;
}

// One launch = one whole MCMC step of B chains (see FusedArgs::step_*).  part: 2 * ceil(B / cpw) floats of scratch.
// The launches of one MCMC step over `rows_all` chain-rows (see launch_fused_step): at most three {rows, rows per
// workgroup} parts, every cut at an even row count.  forms = the sub-tile and 32-row forms may be used.
struct StepPart { int64_t rows; int rpw; };
static int plan_step_parts(int64_t rows_all, bool forms, int cus, StepPart (&parts)[3]) {
  int n = 0;
  if (!forms) {
    parts[n++] = {rows_all, kFM};
  } else if (const int all = fused4_rows_per_wg(rows_all, cus)) {
    parts[n++] = {rows_all, all};
  } else {
    const int64_t round16 = (int64_t)kFM * cus;                          // rows in one full round of 16-row workgroups
    const int64_t main32 = rows_all / (2 * round16) * (2 * round16), rem = rows_all - main32;
    const int64_t over = rem - round16;                                  // rows beyond one more 16-row round
    if (rem > round16 && !(over <= 8 * (int64_t)cus && fused4_rows_per_wg(over, cus))) {
      parts[n++] = {rows_all, 32};                                       // the rest fills most of another 32-row round
    } else {
      if (main32 > 0) parts[n++] = {main32, 32};
      if (rem > round16) {
        parts[n++] = {round16, kFM};
        parts[n++] = {over, fused4_rows_per_wg(over, cus)};
      } else if (rem > 0) {
        const int sub = fused4_rows_per_wg(rem, cus);
        parts[n++] = {rem, sub ? sub : kFM};
      }
    }
  }
  return n;
}
// host logic only, no device call: the launch plan for `rows_all` rows on `cus` CUs
extern "C" int l2hmc_gauge_step_plan(int64_t rows_all, int32_t cus, int64_t* rows_out, int32_t* rpw_out) {
  if (rows_all <= 0 || cus <= 0 || !rows_out || !rpw_out) {
    set_error("gauge_step_plan: rows_all=%lld cus=%d (both > 0) and two output arrays of 3 entries", (long long)rows_all, cus);
    return L2HMC_ERR_ARG;
  }
  StepPart parts[3];
  const int n = plan_step_parts(rows_all, true, cus, parts);
  for (int i = 0; i < n; ++i) {
    rows_out[i] = parts[i].rows;
    rpw_out[i] = parts[i].rpw;
  }
  return n;
}

// hand-off workspace of the split 16-row form: a ticket per pair, then [workgroups][2 * 16 * D + 16] floats
static size_t hand_ticket_bytes(int64_t pairs) { return align_up(sizeof(int) * (size_t)pairs, 256); }
size_t fused_step_hand_bytes(int64_t B, int D) {
  const int64_t pairs = ceil_div(B, (int64_t)kFM);
  return hand_ticket_bytes(pairs) + sizeof(float) * (size_t)(2 * pairs) * (2 * kFM * (size_t)D + kFM);
}

int launch_fused_step(const l2hmc_gauge_plan* p, float beta, const float* x_in, float* x_next, int64_t B,
                      uint64_t seed, uint64_t draw, int both, float* px, float* actions, float* plaqs, float* charges,
                      float* dq, float* step_sums, float* part, void* hand, hipStream_t stream, float* x_prop,
                      float* v_prop, float* x_out, const float* betas, int64_t chain_stride) {
  if (fused_ncp_plan(p)) {
    // torus-exact plans: ONE launch of their own kernel (fused_traj_ncp.hip) for the whole batch -- 8 chains x both
    // directions or 16 chains per workgroup; no parts, no split form, no heads image, no ticket to clear
    L2HMC_REQUIRE(x_in && (x_next || x_out) && B > 0 && (!step_sums || part), "fused step: bad arguments");
    const int cpw = both ? kFM / 2 : kFM;
    FusedArgs a{};
    a.T = p->T; a.X = p->X; a.num_steps = p->num_steps; a.step_begin = 0; a.step_end = p->num_steps;
    a.eps = p->eps; a.beta = beta; a.masks = p->masks; a.xnet = p->xnet; a.vnet = p->vnet;
    a.x0 = x_in; a.rows = ceil_div(B, (int64_t)cpw) * kFM;
    a.step_x_next = x_next; a.step_xprop = x_prop; a.step_vprop = v_prop; a.step_xout = x_out;
    a.step_B = B; a.step_Bl = B; a.step_chain0 = 0; a.step_sums_acc = 0;
    a.step_seed = seed; a.step_draw = draw; a.step_both = both;
    a.step_betas = betas; a.step_beta_stride = chain_stride;
    a.step_px = px; a.step_act = actions; a.step_plq = plaqs; a.step_chg = charges; a.step_dq = dq;
    a.step_sums = step_sums; a.step_part = part;
    return launch_fused_ncp(a, (p->flags & L2HMC_PLAN_RECOMPUTE) != 0, stream);
  }
  const bool conv = (p->flags & L2HMC_PLAN_CONV3D) != 0;
  using CfgG = FusedCfg<128, 512, 128, false>;
  using CfgC = FusedCfg<128, 256, 64, true>;
  static DeviceOnce step_once;
  const size_t lds = sizeof(float) * (conv ? CfgC::LDS_FLOATS : CfgG::LDS_FLOATS);
  if (step_once.pending()) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&gauge_traj_fused_kernel<128, 512, 128, false>),
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(sizeof(float) * CfgG::LDS_FLOATS)) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void*>(&gauge_traj_fused_kernel<128, 256, 64, true>),
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(sizeof(float) * CfgC::LDS_FLOATS)) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void*>(&gauge_traj_fused_kernel<128, 512, 128, false, false, true>),
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(sizeof(float) * CfgG::LDS_FLOATS)) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void*>(&gauge_traj_fused_kernel<128, 256, 64, true, false, true>),
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(sizeof(float) * CfgC::LDS_FLOATS)) != hipSuccess) {
      set_error("fused step: cannot reserve %zu B of LDS", lds);
      return L2HMC_ERR_HIP;
    }
    step_once.done();
  }
  L2HMC_REQUIRE(x_in && (x_next || x_out) && B > 0 && (!step_sums || part) && hand, "fused step: bad arguments");
  // Which form runs which chains (GenericNet 8x8 plans; all forms give the same bits).  The 16-row form covers
  // 16 * (number of CUs) rows per round of workgroups (1.58 ms at the benchmark dynamics), so a batch one chain past a
  // round costs a whole further round.  The batch is cut into at most three parts, launched one after the other on the
  // same stream (a part: chains [c0, c0 + n), global chain indices for the Philox streams, pointers moved to its first
  // chain, the step's sums added to the earlier parts'):
  //   - whole rounds of 32-row workgroups (fused_traj32.hip: twice the rows of a 16-row round in 1.87 x its time);
  //   - what is left: nothing / a sub-tile launch (fused_traj4.hip: up to 3072 rows in 0.9-1.5 ms) / one 16-row round /
  //     a 16-row round and a sub-tile launch (when the rest beyond the round is small) / one more 32-row round;
  //   - a batch that is small as a whole is one sub-tile launch, a batch of at most one round one 16-row launch.
  const int ndir = both ? 2 : 1;
  StepPart parts[3];
  const int nparts = plan_step_parts(B * ndir, !conv && subtile_enabled(p), device_cu_count(), parts);
  auto part_of = [&](int64_t c0, int64_t nb, int rpw, int accumulate) {
    const int cpw = both ? rpw / 2 : rpw;
    const int64_t D = 2 * (int64_t)p->T * p->X;
    FusedArgs a{};
    a.T = p->T; a.X = p->X; a.num_steps = p->num_steps; a.step_begin = 0; a.step_end = p->num_steps;
    a.eps = p->eps; a.beta = beta; a.masks = p->masks; a.xnet = p->xnet; a.vnet = p->vnet;
    a.xfront = p->xfront; a.vfront = p->vfront;
    a.x0 = x_in + c0 * D; a.rows = ceil_div(nb, cpw) * rpw;
    a.step_x_next = x_next ? x_next + c0 * D : nullptr;
    a.step_xprop = x_prop ? x_prop + c0 * D : nullptr;
    a.step_vprop = v_prop ? v_prop + c0 * D : nullptr;
    a.step_xout = x_out ? x_out + c0 * D : nullptr;
    a.step_B = B; a.step_Bl = nb; a.step_chain0 = c0; a.step_sums_acc = accumulate;
    a.step_seed = seed; a.step_draw = draw; a.step_both = both;
    a.step_betas = betas ? betas + c0 * chain_stride : nullptr; a.step_beta_stride = chain_stride;   // (a ladder)
    a.step_px = px ? px + c0 : nullptr; a.step_act = actions ? actions + c0 : nullptr;
    a.step_plq = plaqs ? plaqs + c0 : nullptr; a.step_chg = charges ? charges + c0 : nullptr;
    a.step_dq = dq ? dq + c0 : nullptr;
    a.step_sums = step_sums; a.step_part = part;
    a.single_kicks = (p->flags & L2HMC_PLAN_SINGLE_KICKS) != 0;
#ifdef L2HMC_STAMPS
    a.stamps = g_stamp_cls == 5 ? g_stamp_buf : nullptr;
    a.stagger = g_fused_stagger;
#endif
    return a;
  };
  // GenericNet, both directions: the split form (FusedArgs::step_split), with the active-column heads unless the plan
  // has none or asks for all columns (L2HMC_PLAN_ALL_COLUMNS)
  const bool split = !conv && both;
  // ... and the first layer's x product of a position sub-update on the kept columns unless L2HMC_PLAN_FULL_L1
  const int* hmeta = nullptr;
  const float* himg = nullptr;
  const float* l1img = nullptr;
  if (split && p->heads && !(p->flags & L2HMC_PLAN_ALL_COLUMNS)) {
    const int Dp = 2 * p->T * p->X;
    hmeta = reinterpret_cast<const int*>(p->heads);
    himg = reinterpret_cast<const float*>(reinterpret_cast<const char*>(p->heads) + heads_meta_bytes(p->num_steps, Dp));
    if (!(p->flags & L2HMC_PLAN_FULL_L1))
      l1img = reinterpret_cast<const float*>(reinterpret_cast<const char*>(himg) +
                                             heads_sections_bytes(p->num_steps, Dp, p->xnet.H));
  }
  auto launch16 = [&](FusedArgs a) {
    if (split) {
      const int64_t pairs = ceil_div(a.step_Bl, (int64_t)kFM);
      a.rows = 2 * pairs * kFM;
      a.step_split = 1;
      a.step_ticket = static_cast<int*>(hand);
      a.step_hand = reinterpret_cast<float*>(static_cast<char*>(hand) + hand_ticket_bytes(pairs));
      a.heads_meta = hmeta;
      a.heads_img = himg;
      a.l1_img = l1img;
      // the tickets are cleared by a kernel of the step itself, never by a memset: a captured step is kernel nodes
      // only, each ordered behind the one before it, and the workspace may hold anything on entry
      hipLaunchKernelGGL(clear_tickets_kernel, dim3((unsigned)ceil_div(pairs, (int64_t)256)), dim3(256), 0, stream,
                         a.step_ticket, pairs);
      L2HMC_CHECK_LAUNCH("fused step: clear of the hand-off tickets");
    }
    const unsigned nwg = (unsigned)(a.rows / kFM);
    prof_before(kProfFused, stream);
    if (conv && a.step_betas)
      hipLaunchKernelGGL((gauge_traj_fused_kernel<128, 256, 64, true, false, true>), dim3(nwg), dim3(CfgC::THREADS), lds,
                         stream, a);
    else if (conv)
      hipLaunchKernelGGL((gauge_traj_fused_kernel<128, 256, 64, true>), dim3(nwg), dim3(CfgC::THREADS), lds, stream, a);
    else if (a.step_betas)
      hipLaunchKernelGGL((gauge_traj_fused_kernel<128, 512, 128, false, false, true>), dim3(nwg), dim3(CfgG::THREADS), lds,
                         stream, a);
    else
      hipLaunchKernelGGL((gauge_traj_fused_kernel<128, 512, 128, false>), dim3(nwg), dim3(CfgG::THREADS), lds, stream, a);
    prof_after(kProfFused, stream);
    L2HMC_CHECK_LAUNCH("gauge_traj_fused (step)");
    return L2HMC_OK;
  };
  int64_t c0 = 0;
  for (int i = 0; i < nparts; ++i) {
    const int64_t nb = parts[i].rows / ndir;                             // (every cut is at an even row count)
    const FusedArgs a = part_of(c0, nb, parts[i].rpw, i > 0);
    if (int e = parts[i].rpw == 32 ? launch_fused32(a, stream)
                : parts[i].rpw == kFM ? launch16(a) : launch_fused4(a, parts[i].rpw, stream))
      return e;
    c0 += nb;
  }
  return L2HMC_OK;
}

}  // namespace l2hmc

using namespace l2hmc;

extern "C" size_t l2hmc_gauge_pack_heads_bytes(const l2hmc_gauge_plan* plan) {
  if (!plan || plan->hmc || plan->num_steps <= 0 || (plan->flags & L2HMC_PLAN_CONV3D) || 2 * plan->T * plan->X != 128 ||
      !fused_generic_net(&plan->xnet))
    return 0;
  const int D = 128, H = plan->xnet.H;
  return heads_meta_bytes(plan->num_steps, D) + heads_sections_bytes(plan->num_steps, D, H) +
         l1_sections_bytes(plan->num_steps, D, H);
}

extern "C" int l2hmc_gauge_pack_heads(const l2hmc_gauge_plan* plan, void* buf, l2hmc_stream_t stream) {
  L2HMC_REQUIRE(plan != nullptr && buf != nullptr, "gauge_pack_heads: NULL pointer");
  L2HMC_REQUIRE(l2hmc_gauge_pack_heads_bytes(plan) > 0, "gauge_pack_heads: the plan has no active-column heads "
                "(GenericNet D = 128, H = 512 on an 8x8-site lattice, hmc = 0)");
  L2HMC_REQUIRE(plan->masks && plan->xnet.whd_t && plan->xnet.w1_t, "gauge_pack_heads: NULL masks or weights");
  const int N = plan->num_steps, D = 128;
  int* meta = static_cast<int*>(buf);
  float* img = reinterpret_cast<float*>(static_cast<char*>(buf) + heads_meta_bytes(N, D));
  float* img1 = reinterpret_cast<float*>(reinterpret_cast<char*>(img) + heads_sections_bytes(N, D, plan->xnet.H));
  hipLaunchKernelGGL(pack_heads_kernel, dim3(32, (unsigned)(2 * N)), dim3(256), 0, (hipStream_t)stream, plan->xnet,
                     plan->masks, N, meta, img, meta + 2 * N + N * D, img1);
  L2HMC_CHECK_LAUNCH("gauge_pack_heads");
  return L2HMC_OK;
}

extern "C" size_t l2hmc_dense_pack_bytes(const l2hmc_dense_net* net) {
  if (!net || !fused_net_supported(net)) return 0;
  // the 16-row form's image, then (GenericNet plans) the sub-tile form's (fused_traj4.hip)
  return sizeof(float) * ((size_t)(net->Ka + net->Kb) * net->H + (size_t)net->H * net->H + (size_t)3 * net->D * net->H +
                          fused4_pack_floats(net));
}

extern "C" int l2hmc_dense_pack(const l2hmc_dense_net* net, float* packed, l2hmc_stream_t stream) {
  L2HMC_REQUIRE(net != nullptr && packed != nullptr, "dense_pack: NULL pointer");
  L2HMC_REQUIRE(fused_net_supported(net), "dense_pack: shape (D=%d, H=%d, Ka=%d, Kb=%d) has no fused kernel",
                net->D, net->H, net->Ka, net->Kb);
  L2HMC_REQUIRE(net->w1_t && net->wh_t && net->whd_t, "dense_pack: NULL weight pointer");
  const int waves = fused_conv_net(net) ? FusedCfg<128, 256, 64, true>::IMGW : FusedCfg<128, 512, 128, false>::IMGW;
  hipLaunchKernelGGL(pack_fused_kernel, dim3(1024), dim3(256), 0, (hipStream_t)stream, *net, packed, waves);
  L2HMC_CHECK_LAUNCH("dense_pack");
  if (fused4_pack_floats(net))
    return launch_fused4_pack(net, packed + (size_t)(net->Ka + net->Kb) * net->H + (size_t)net->H * net->H +
                                        (size_t)3 * net->D * net->H, (hipStream_t)stream);
  return L2HMC_OK;
}
