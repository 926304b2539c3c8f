// Whole-step kernel of the torus-exact L2HMC mode (L2HMC_PLAN_PERIODIC | L2HMC_PLAN_PERIODIC_STEP) on D = 128 (gfx950).
//
// One launch integrates all leapfrog steps of a periodic plan for a tile of 16 chain-rows per workgroup, as
// gauge_traj_fused_kernel (fused_traj.hip) does for the reference mode, and finishes the MCMC step in step mode.  What
// differs from that kernel:
//   - the networks read the links through [cos x | sin x]: a feature buffer fs [16][2 D + 8] in LDS, and first layers
//     of K = 3 D = 24 k-chunks in the order of the packed image (pack_fused_kernel walks Ka, then Kb):
//       VNet  fs (16 chunks: [cos x | sin x])  then  gs (8 chunks: force),
//       XNet  vs (8 chunks)  then  fs (16 chunks: keep (.) [cos x | sin x], the keep mask on both halves);
//   - the position sub-update is lf_drift_ncp (lf_update.h): the scaling acts on the circle;
//   - the features are formed where x changes: at the start (unmasked, for VNet's first call), in a kick's epilogue
//     (the stored features times the keep of position sub-update 1: x has not moved since they were formed), behind
//     sub-update 1 (the new x under the complementary keep; a kept column has its x unchanged but its mask value
//     changed, so every column is rewritten) and behind sub-update 2 (unmasked, for the kick that follows).  libm
//     sincosf, as l2hmc_u1_angle_features.
// One form only: 16 rows per workgroup (8 chains x both directions, or 16 chains with L2HMC_PLAN_SELECTED_ONLY),
// every batch as ceil(rows / 16) workgroups; no split form, no active-column heads, no kept-column first layer, no
// paired half-kicks, no sub-tile or 32-row sibling; the training tape in instances of their own (TAPE, below: the
// forward of l2hmc_gauge_train_forward[_ladder] on a plan with L2HMC_PLAN_PERIODIC_TAPE).  The chain-local and step
// stages are fused_step.h's, the streaming products fused_common.h's, the sub-update arithmetic lf_update.h's.
//
// Waves: 8 on the 4-wave image (two per SIMD, two per image section: RW = 2), the geometry of the GenericNet
// instances of gauge_traj_fused_kernel, whose measurements (fused_traj.hip, FusedCfg) chose it: one wave's epilogues
// and barriers lie under the other's matrix instructions.  The epilogues here are longer (sincosf, atan2f, logf), which
// argues the same way; a 4-wave build was not measured.
//
// Kept first-layer products (bit-identical to forming them anew: the same accumulator chain continues at the same k):
//   keep_v  VNet's whole product, from call 3 of step s to call 0 of step s + 1 (same x and force, so same features);
//   keep_x  XNet's product over its first 8 chunks (the v half), shared by the two position sub-updates of a step.
// They are never live together and share one register set.  `recompute` (L2HMC_PLAN_RECOMPUTE) switches them off.
#include "fused_step.h"
#include "lf_update.h"

namespace l2hmc {

struct NcpCfg {
  static constexpr int D = 128, H = 512;
  static constexpr int IMGW = 4, WAVES = 8, RW = WAVES / IMGW, THREADS = 64 * WAVES;
  static constexpr int TPC = 16;                   // threads per chain in the chain-local passes (every GenericNet form)
  static constexpr int SX = D + 8, SH = H + 8, SF = 2 * D + 8;     // LDS row strides: x / v / force, h1 / h2, features
  static constexpr int NT1 = H / (16 * WAVES);     // 16-column tiles per wave, layers 1 and 2
  static constexpr int NTI1 = H / (16 * IMGW);     // ... and per image section
  static constexpr int NTIH = D / (16 * IMGW);     // tiles per head in an image section; a wave takes one of them
  static_assert(D / (16 * WAVES) == 1, "one heads tile per wave");
  static constexpr int KCD = D / 16;               // k-chunks of a D-wide first-layer input (v, force)
  static constexpr int KC1 = 3 * KCD;              // first layer: K = 3 D
  static constexpr int KC2 = H / 16;
  static constexpr size_t P1 = (size_t)3 * D * H, P2 = (size_t)H * H;
  static constexpr int NC = 4 * H + 5 * D;         // per-net constants (load_consts)
  static constexpr int SP = D / 2 + 4;
  static constexpr int LDS_FLOATS = 3 * kFM * SX + 2 * kFM * SH + 2 * NC + kFM * SP + 2 * D /*masks*/ +
                                    WAVES * kFM /*ldw*/ + kFM /*dir*/ + 8 * kFM /*step mode*/ + kFM * SF /*features*/;
  static_assert(LDS_FLOATS * sizeof(float) <= 160 * 1024, "one workgroup must fit the LDS of a CU");
};

// TAPE: the training instances (L2HMC_PLAN_PERIODIC_TAPE; trajectory mode only), which also write the per-call tape of
// train.hip's taped_call for a torus-exact plan -- in [3 D], st, h1, h2 and the S / T / Q planes, not the gate words
// (their only reader is the reference mode's fused reverse kernel).  Taping only adds stores: the bits are the untaped
// instance's.  TAPE && LADDER: the taped forward of a training step on a ladder (a beta per row; fused_step.h).
// The taped instances keep the first-layer products too.  With keep_v / keep_x alive across the tape stores they sit at
// 256 VGPRs with 76 - 80 B of scratch, and three (LADDER: four) spilled loop-invariant values are reloaded at the head
// of every leapfrog step, none inside the four-call loop; without the kept products (L2HMC_NCP_TAPE_KEPT = 0: 234 - 235
// VGPRs, no scratch at all, the same bits) the launch measured 8 % slower (profiles/periodic_train_forward.txt (c)).
#ifndef L2HMC_NCP_TAPE_KEPT
#define L2HMC_NCP_TAPE_KEPT 1
#endif
template <bool LADDER, bool TAPE = false>
__global__ __launch_bounds__(NcpCfg::THREADS) void gauge_traj_ncp_kernel(FusedArgs p, int recompute) {
  using Cfg = NcpCfg;
  constexpr bool KEPT = !TAPE || L2HMC_NCP_TAPE_KEPT;
  constexpr int D = Cfg::D, H = Cfg::H, kThreads = Cfg::THREADS, kTPC = Cfg::TPC, kWaves = Cfg::WAVES;
  constexpr int SX = Cfg::SX, SH = Cfg::SH, SF = Cfg::SF, SP = Cfg::SP, NT1 = Cfg::NT1, NTI1 = Cfg::NTI1;
  constexpr int NTIH = Cfg::NTIH, RW = Cfg::RW, KCD = Cfg::KCD;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xs = lds;                         // [16][SX] position
  float* vs = xs + kFM * SX;               // [16][SX] momentum
  float* gs = vs + kFM * SX;               // [16][SX] force
  float* h1 = gs + kFM * SX;               // [16][SH]
  float* h2 = h1 + kFM * SH;               // [16][SH]
  float* cx = h2 + kFM * SH;               // XNet constants [NC]
  float* cv = cx + Cfg::NC;                // VNet constants [NC]
  float* sp = cv + Cfg::NC;                // [16][SP] sin P
  float* skm = sp + kFM * SP;              // [2][D] masks of this step: forward row, backward row
  float* ldw = skm + 2 * D;                // [WAVES][16] log-det partial sums per wave
  int* sdir = reinterpret_cast<int*>(ldw + kWaves * kFM);   // [16]
  float* stp = reinterpret_cast<float*>(sdir + kFM);        // step mode: coin[16] u[16] p_row[16] obs[16][4] beta[16]
  float* fs = stp + 8 * kFM;               // [16][SF] [cos x | sin x], unmasked or under the keep of the next XNet call

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int q = lane >> 4, r = lane & 15;
  const float eps = p.eps;

  // ---- stage chain state, constants and the features of x0 (fused_step.h) ------
  const StepWg wg = step_workgroup<kFM>(p, stp, false);
  stage_chains<kFM, kThreads, D, SX, LADDER, TAPE>(p, wg, xs, vs, sdir);
  load_consts<kThreads, D, H>(p.xnet, cx, tid);
  load_consts<kThreads, D, H>(p.vnet, cv, tid);
  if (tid < kWaves * kFM) ldw[tid] = 0.f;
  __syncthreads();
  for (int i = tid; i < kFM * D; i += kThreads) {
    const int rr = i / D, c = i - rr * D;
    float sn, cs;
    sincosf(xs[rr * SX + c], &sn, &cs);
    fs[rr * SF + c] = cs;
    fs[rr * SF + D + c] = sn;
  }
  const int dirl = sdir[r];           // direction of the row this lane owns in a C fragment (fused_common.h)

  const ChainLanes cl = chain_lanes<kFM, kTPC, 1>(p, wg, tid);
  float act0[1], kin0[1];
  force_pass<kFM, kTPC, 1, D, SX, SP, LADDER>(cl, xs, sp, gs, act0);     // leaves the force of x0 in gs; ends in a barrier
  kinetic_pass<kFM, kTPC, 1, D, SX>(cl, vs, kin0);

  f32x4 keep[NT1];                    // keep_x (call 1 -> call 2) or keep_v (call 3 -> the next step's call 0)

  // ---- one network evaluation + fused sub-update ------------------------------
  // VNet (kick; sub = 0: the step's first, 1: its second): inputs fs, gs.  XNet (position sub-update `sub`): inputs vs, fs.
  // l1: 0 = form the whole product; 1 = as 0 and keep it (keep_v); 2 = take keep_v, no product;
  //     3 = keep the product over the first input (keep_x); 4 = start from keep_x, second input only.
  auto net_update = [&](const l2hmc_dense_net& net, const float* cn, bool is_vnet, int sub, int l1, const float tcr,
                        const float tsr, int callidx) {
    const float* pk = net.packed;
    const bool zig = (callidx & 1) != 0;                      // layers 2 and 3 alternate their direction (fused_common.h)
    // training tape: this call's input rows as the first layer reads them and the state its sub-update consumes.  The
    // inputs are complete behind the barrier that ended the previous stage, also where no product is formed from them
    // (l1 == 2), and VNet's features leave here UNMASKED: this call's own epilogue puts the next keep on fs two
    // barriers further on.
    [[maybe_unused]] const FusedTape& tp = is_vnet ? p.tv : p.tx;
    [[maybe_unused]] const size_t tcr0 = (size_t)callidx * (size_t)p.rows + (size_t)wg.row0;   // first taped row of this workgroup
    if constexpr (TAPE) {
      const float* stsrc = is_vnet ? vs : xs;
      for (int i = tid; i < kFM * (D / 4); i += kThreads) {
        const int rr = i / (D / 4), c4 = (i - rr * (D / 4)) * 4;
        if (rr < wg.nrow) {
          float* dst = tp.in + (tcr0 + rr) * (3 * D);
          const f32x4 fc = *reinterpret_cast<const f32x4*>(fs + rr * SF + c4);
          const f32x4 fn = *reinterpret_cast<const f32x4*>(fs + rr * SF + D + c4);
          if (is_vnet) {          // [cos x | sin x | beta force]
            tape_store(dst + c4, fc);
            tape_store(dst + D + c4, fn);
            tape_store(dst + 2 * D + c4, *reinterpret_cast<const f32x4*>(gs + rr * SX + c4));
          } else {                // [v | keep cos x | keep sin x]
            tape_store(dst + c4, *reinterpret_cast<const f32x4*>(vs + rr * SX + c4));
            tape_store(dst + D + c4, fc);
            tape_store(dst + 2 * D + c4, fn);
          }
          tape_store(tp.st + (tcr0 + rr) * D + c4, *reinterpret_cast<const f32x4*>(stsrc + rr * SX + c4));
        }
      }
    }
    [[maybe_unused]] auto tape_rows = [&](float* dst, const float* src) {     // [16][H] LDS rows -> tape
      for (int i = tid; i < kFM * (H / 4); i += kThreads) {
        const int rr = i / (H / 4), c4 = (i - rr * (H / 4)) * 4;
        if (rr < wg.nrow) tape_store(dst + (tcr0 + rr) * H + c4, *reinterpret_cast<const f32x4*>(src + rr * SH + c4));
      }
    };
    const int wv = __builtin_amdgcn_readfirstlane(wave);      // wave-uniform: the weight loads' base stays in SGPRs
    const int wimg = wv / RW, wsub = wv - wimg * RW;          // image section, and this wave's share of it
    const float* wp1 = pk + (size_t)wimg * Cfg::KC1 * NTI1 * 256;
    const float* wp2 = pk + Cfg::P1 + (size_t)wimg * Cfg::KC2 * NTI1 * 256;
    const float* wph = pk + Cfg::P1 + Cfg::P2 + (size_t)wimg * Cfg::KC2 * 3 * NTIH * 256;
    const int to1 = wsub * NT1, toh = wsub;                   // first tile of this wave in a chunk of the section
    constexpr int DP1 = 3, DP2 = 3, DPH = 4;                  // ring depths: first-layer parts, layer 2, heads
    BRing<NT1, DP2> R2;
    BRing<3, DPH> R3;
    // ----- layer 1: the first input's chunks, then the second input's
    {
      f32x4 acc[NT1];
      if (l1 == 2) {
#pragma unroll
        for (int t = 0; t < NT1; ++t) acc[t] = keep[t];
      } else {
        BRing<NT1, DP1> RA, RB;
        const float* wpb = wp1 + (size_t)(is_vnet ? 2 * KCD : KCD) * NTI1 * 256;
        ring_prime<NT1, DP1, NTI1>(RB, wpb, false, 0, to1);         // both parts' first fragments are requested up front
        if (l1 == 4) {
#pragma unroll
          for (int t = 0; t < NT1; ++t) acc[t] = keep[t];
        } else {
          ring_prime<NT1, DP1, NTI1>(RA, wp1, false, 0, to1);
#pragma unroll
          for (int t = 0; t < NT1; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        if (is_vnet) {
          const float* a1 = fs + r * SF + q * 4;
          stream_layer<NT1, 2 * KCD, DP1, NTI1>(
              RA, wp1, [&](int kc) { return *reinterpret_cast<const f32x4*>(a1 + kc * 16); }, acc, false, to1);
          const float* a2 = gs + r * SX + q * 4;
          stream_layer<NT1, KCD, DP1, NTI1>(
              RB, wpb, [&](int kc) { return *reinterpret_cast<const f32x4*>(a2 + kc * 16); }, acc, false, to1);
          if (l1 == 1) {
#pragma unroll
            for (int t = 0; t < NT1; ++t) keep[t] = acc[t];
          }
        } else {
          if (l1 != 4) {
            const float* a1 = vs + r * SX + q * 4;
            stream_layer<NT1, KCD, DP1, NTI1>(
                RA, wp1, [&](int kc) { return *reinterpret_cast<const f32x4*>(a1 + kc * 16); }, acc, false, to1);
            if (l1 == 3) {
#pragma unroll
              for (int t = 0; t < NT1; ++t) keep[t] = acc[t];
            }
          }
          const float* a2 = fs + r * SF + q * 4;
          stream_layer<NT1, 2 * KCD, DP1, NTI1>(
              RB, wpb, [&](int kc) { return *reinterpret_cast<const f32x4*>(a2 + kc * 16); }, acc, false, to1);
        }
      }
      ring_prime<NT1, DP2, NTI1>(R2, wp2, zig, Cfg::KC2, to1);      // layer-2 weights start flowing under the epilogue + barrier
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
      }
    }
    __syncthreads();
    if constexpr (TAPE) tape_rows(tp.h1, h1);
    // ----- layer 2
    {
      f32x4 acc[NT1];
#pragma unroll
      for (int t = 0; t < NT1; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      const float* a = h1 + r * SH + q * 4;
      stream_layer<NT1, Cfg::KC2, DP2, NTI1>(
          R2, wp2, [&](int kc) { return *reinterpret_cast<const f32x4*>(a + kc * 16); }, acc, zig, to1);
      ring_prime<3, DPH, 3 * NTIH, NTIH>(R3, wph, zig, Cfg::KC2, toh);
#pragma unroll
      for (int t = 0; t < NT1; ++t) {
        const int c0 = (wave * NT1 + t) * 16 + q * 4;
        const f32x4 b = *reinterpret_cast<const f32x4*>(cn + 3 * H + c0);
        f32x4 hv;
#pragma unroll
        for (int e = 0; e < 4; ++e) hv[e] = relu_nan(acc[t][e] + b[e]);
        *reinterpret_cast<f32x4*>(h2 + r * SH + c0) = hv;
      }
    }
    __syncthreads();
    if constexpr (TAPE) tape_rows(tp.h2, h2);
    // ----- heads + update: this wave's 16 columns [S | T | Q] of row r
    {
      f32x4 acc[3];
#pragma unroll
      for (int t = 0; t < 3; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      const float* a = h2 + r * SH + q * 4;
      stream_layer<3, Cfg::KC2, DPH, 3 * NTIH, NTIH>(
          R3, wph, [&](int kc) { return *reinterpret_cast<const f32x4*>(a + kc * 16); }, acc, zig, toh);
      float ld = 0.f;                       // this lane's share of row r's log-det
      const float* bhd = cn + 4 * H;
      const float* es = bhd + 3 * D;
      const float* eq = es + D;
      const int d = dirl;
      const int c0 = wave * 16 + q * 4;     // row r, columns c0 .. c0 + 3
      const f32x4 b_s = *reinterpret_cast<const f32x4*>(bhd + c0);
      const f32x4 b_t = *reinterpret_cast<const f32x4*>(bhd + D + c0);
      const f32x4 b_q = *reinterpret_cast<const f32x4*>(bhd + 2 * D + c0);
      const f32x4 e_s = *reinterpret_cast<const f32x4*>(es + c0);
      const f32x4 e_q = *reinterpret_cast<const f32x4*>(eq + c0);
      const f32x4 mf = *reinterpret_cast<const f32x4*>(skm + c0);
      const f32x4 mb = *reinterpret_cast<const f32x4*>(skm + D + c0);
      const int idx = r * SX + c0, fidx = r * SF + c0;
      f32x4 S, Tt, Q;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float s_, t_, q_;
        heads_stq(acc[0][e], acc[1][e], acc[2][e], b_s[e], b_t[e], b_q[e], e_s[e], e_q[e], net.q_tanh, s_, t_, q_);
        S[e] = s_; Tt[e] = t_; Q[e] = q_;
      }
      if constexpr (TAPE) {
        if (r < wg.nrow) {
          const size_t plane = (size_t)p.rows * D;
          float* o = tp.stq + (size_t)callidx * 3 * plane + ((size_t)wg.row0 + r) * D + c0;
          tape_store(o, S);
          tape_store(o + plane, Tt);
          tape_store(o + 2 * plane, Q);
        }
      }
      if (is_vnet) {
        const f32x4 g = *reinterpret_cast<const f32x4*>(gs + idx);
        const f32x4 v = *reinterpret_cast<const f32x4*>(vs + idx);
        f32x4 vn;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float s;
          vn[e] = lf_kick<ExpFast>(v[e], g[e], S[e], Tt[e], Q[e], eps, d, s);
          ld += s;
        }
        *reinterpret_cast<f32x4*>(vs + idx) = vn;
        // the next call is position sub-update 1 (sub == 0 marks the step's first kick): x has not moved since fs was
        // formed, so the features under that sub-update's keep are the stored ones times the keep, on both halves
        if (sub == 0) {
          f32x4 fc = *reinterpret_cast<const f32x4*>(fs + fidx);
          f32x4 fn = *reinterpret_cast<const f32x4*>(fs + fidx + D);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float k = keep_of(mf[e], mb[e], d, 0);
            fc[e] = k * fc[e];
            fn[e] = k * fn[e];
          }
          *reinterpret_cast<f32x4*>(fs + fidx) = fc;
          *reinterpret_cast<f32x4*>(fs + fidx + D) = fn;
        }
      } else {
        const f32x4 x = *reinterpret_cast<const f32x4*>(xs + idx);
        const f32x4 v = *reinterpret_cast<const f32x4*>(vs + idx);
        f32x4 xn, fc, fn;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float s, omk;
          xn[e] = lf_drift_ncp<ExpFast>(x[e], v[e], keep_of(mf[e], mb[e], d, sub), S[e], Tt[e], Q[e], eps, d, s, omk);
          ld += omk * s;
          // features of the new x: under the complementary keep for sub-update 2, unmasked for the kick behind it
          float sn, cs;
          sincosf(xn[e], &sn, &cs);
          if (sub == 0) {
            const float k = keep_of(mf[e], mb[e], d, 1);
            cs = k * cs;
            sn = k * sn;
          }
          fc[e] = cs;
          fn[e] = sn;
        }
        *reinterpret_cast<f32x4*>(xs + idx) = xn;
        *reinterpret_cast<f32x4*>(fs + fidx) = fc;
        *reinterpret_cast<f32x4*>(fs + fidx + D) = fn;
      }
      // row r's log-det share of this wave: lanes r, r + 16, r + 32, r + 48 (fixed order: bit-reproducible)
      ld += __shfl_xor(ld, 16, 64);
      ld += __shfl_xor(ld, 32, 64);
      if (q == 0) ldw[wave * kFM + r] += ld;
    }
    __syncthreads();
  };

  // ---- leapfrog steps -----------------------------------------------------------
  const float two_pi = 6.28318530717958647692f;
  bool keep_v_valid = false;
  for (int step = p.step_begin; step < p.step_end; ++step) {
    // time encoding of this lane's row and the masks of the step (gauge_dynamics.py:453-457): forward rows take step,
    // backward rows num_steps - 1 - step
    const int sf = step, sb = p.num_steps - 1 - step;
    const float af = two_pi * (float)sf / (float)p.num_steps, ab = two_pi * (float)sb / (float)p.num_steps;
    const float tcr = dirl ? cosf(ab) : cosf(af), tsr = dirl ? sinf(ab) : sinf(af);
    for (int i = tid; i < D; i += kThreads) {
      skm[i] = p.masks[(size_t)sf * D + i];
      skm[D + i] = p.masks[(size_t)sb * D + i];
    }
    __syncthreads();
    // the four network calls of a leapfrog step run through ONE copy of the code (wave-uniform branches)
#pragma nounroll
    for (int call = 0; call < 4; ++call) {
      const bool is_v = call == 0 || call == 3;
      if (call == 3) {
        float unused[1];
        force_pass<kFM, kTPC, 1, D, SX, SP, LADDER>(cl, xs, sp, gs, unused);   // force at the new position
      }
      // call 0: momentum half-kick (+ masked features)         call 1: position sub-update 1 (+ complement mask)
      // call 2: position sub-update 2 (+ unmasked features)    call 3: second momentum half-kick (product kept)
      const int l1 = (!KEPT || recompute) ? 0 : call == 0 ? (keep_v_valid ? 2 : 0) : call == 1 ? 3 : call == 2 ? 4 : 1;
      net_update(is_v ? p.vnet : p.xnet, is_v ? cv : cx, is_v, /*sub=*/call >> 1, l1, tcr, tsr, 2 * step + (call >> 1));
    }
    keep_v_valid = !recompute;
  }

  // ---- epilogue: energies, accept probability, write back -------------------------
  float act1[1], kin1[1];
  force_pass<kFM, kTPC, 1, D, SX, SP, LADDER>(cl, xs, sp, gs, act1);
  kinetic_pass<kFM, kTPC, 1, D, SX>(cl, vs, kin1);
  if (!TAPE && wg.stepm) {              // (the taped instances are trajectory mode only)
    float* spx = wg.spx;
    step_accept_probs<kFM, 1, kWaves, LADDER>(cl, ldw, act0, act1, kin0, kin1, spx);
    __syncthreads();
    // mix, accept, measure, sum, wrap (fused_step.h); x_in -> gs rows, x_out -> h1 rows (both free now)
    float* gin = gs;
    float* gout = h1;
    step_mix_accept<kThreads, D, SX>(p, wg, xs, xs + (kFM / 2) * SX, vs, vs + (kFM / 2) * SX, spx, spx + kFM / 2, gin,
                                     gout);
    step_observables<kFM, kTPC, 1, D, SX>(p, wg, cl, gin, gout);
    step_sums<kThreads, kThreads>(p, wg, 1, (int64_t)blockIdx.x, (int)gridDim.x, (int)gridDim.x, /*fin=*/vs);   // (vs is dead)
    step_write_next<kThreads, D, SX>(p, wg, gout);
    return;
  }
  traj_logdet_accept<kFM, 1, kWaves, TAPE && LADDER>(p, wg, cl, ldw, act0, act1, kin0, kin1);
  traj_write_back<kFM, kThreads, D, SX>(p, wg, xs, vs);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// the two network shapes of a periodic plan at D = 128: XNet (v | keep (.) features), VNet (features | force)
static int ncp_xnet(const l2hmc_dense_net* n) { return n->D == 128 && n->H == 512 && n->Ka == 128 && n->Kb == 256; }
static int ncp_vnet(const l2hmc_dense_net* n) { return n->D == 128 && n->H == 512 && n->Ka == 256 && n->Kb == 128; }
int fused_ncp_net_supported(const l2hmc_dense_net* n) { return ncp_xnet(n) || ncp_vnet(n); }

// the shapes the kernel serves, whatever asks for it
static int ncp_shape(const l2hmc_gauge_plan* p) {
  return !p->hmc && !(p->flags & L2HMC_PLAN_CONV3D) && 2 * p->T * p->X == 128 && (p->X & (p->X - 1)) == 0 &&
         ncp_xnet(&p->xnet) && ncp_vnet(&p->vnet) && p->xnet.packed && p->vnet.packed;
}

int fused_ncp_plan(const l2hmc_gauge_plan* p) {
  const int both = L2HMC_PLAN_PERIODIC | L2HMC_PLAN_PERIODIC_STEP;
  return (p->flags & both) == both && ncp_shape(p);
}

// the taped instances: the training forward of a plan with L2HMC_PLAN_PERIODIC_TAPE (no L2HMC_PLAN_PERIODIC_STEP needed;
// L2HMC_PLAN_LAYERED wins)
int fused_ncp_tape_plan(const l2hmc_gauge_plan* p) {
  const int all = L2HMC_PLAN_PERIODIC | L2HMC_PLAN_PERIODIC_TRAIN | L2HMC_PLAN_PERIODIC_TAPE;
  return (p->flags & all) == all && !(p->flags & L2HMC_PLAN_LAYERED) && ncp_shape(p);
}

// a: the descriptor of launch_fused_trajectory / launch_fused_step (fused_traj.hip), rows a multiple of 16 in step mode.
// a.tx.in set: the taped instances (every tape array of both networks but `gate`, the whole trajectory, trajectory mode).
int launch_fused_ncp(const FusedArgs& a, int recompute, hipStream_t stream) {
  static DeviceOnce once;
  const size_t lds = sizeof(float) * NcpCfg::LDS_FLOATS;
  const bool tape = a.tx.in != nullptr || a.tv.in != nullptr;
  if (tape) {
    static DeviceOnce tape_once;
    if (tape_once.pending()) {
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(&gauge_traj_ncp_kernel<false, true>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess ||
          hipFuncSetAttribute(reinterpret_cast<const void*>(&gauge_traj_ncp_kernel<true, true>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        set_error("fused periodic step: cannot reserve %zu B of LDS", lds);
        return L2HMC_ERR_HIP;
      }
      tape_once.done();
    }
    L2HMC_REQUIRE(a.rows > 0 && a.xnet.packed && a.vnet.packed && a.x0 && a.v0 && a.x_out && a.v_out,
                  "fused periodic step: bad arguments");
    L2HMC_REQUIRE(a.step_B == 0 && a.step_begin == 0 && a.step_end == a.num_steps,
                  "fused periodic step: taping needs trajectory mode and the whole trajectory");
    L2HMC_REQUIRE(a.tx.in && a.tx.h1 && a.tx.h2 && a.tx.stq && a.tx.st && a.tv.in && a.tv.h1 && a.tv.h2 && a.tv.stq &&
                      a.tv.st,
                  "fused periodic step: NULL tape pointer");
    L2HMC_REQUIRE(!a.step_betas || (a.step_beta_mod > 0 && (a.step_beta_stride == 0 || a.step_beta_stride == 1)),
                  "fused periodic step: a beta per row needs a modulus > 0 and an element stride of 0 or 1");
    const dim3 tgrid((unsigned)ceil_div(a.rows, (int64_t)kFM));
    prof_before(kProfFused, stream);
    if (a.step_betas)
      hipLaunchKernelGGL((gauge_traj_ncp_kernel<true, true>), tgrid, dim3(NcpCfg::THREADS), lds, stream, a, recompute);
    else
      hipLaunchKernelGGL((gauge_traj_ncp_kernel<false, true>), tgrid, dim3(NcpCfg::THREADS), lds, stream, a, recompute);
    prof_after(kProfFused, stream);
    L2HMC_CHECK_LAUNCH("gauge_traj_ncp_tape");
    return L2HMC_OK;
  }
  if (once.pending()) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&gauge_traj_ncp_kernel<false>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void*>(&gauge_traj_ncp_kernel<true>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
      set_error("fused periodic step: cannot reserve %zu B of LDS", lds);
      return L2HMC_ERR_HIP;
    }
    once.done();
  }
  L2HMC_REQUIRE(a.rows > 0 && a.xnet.packed && a.vnet.packed, "fused periodic step: bad arguments");
  L2HMC_REQUIRE(!a.step_betas || a.step_B > 0, "fused periodic step: a beta per chain needs step mode");
  const dim3 grid((unsigned)ceil_div(a.rows, (int64_t)kFM));
  prof_before(kProfFused, stream);
  if (a.step_betas)
    hipLaunchKernelGGL(gauge_traj_ncp_kernel<true>, grid, dim3(NcpCfg::THREADS), lds, stream, a, recompute);
  else
    hipLaunchKernelGGL(gauge_traj_ncp_kernel<false>, grid, dim3(NcpCfg::THREADS), lds, stream, a, recompute);
  prof_after(kProfFused, stream);
  L2HMC_CHECK_LAUNCH("gauge_traj_ncp");
  return L2HMC_OK;
}

}  // namespace l2hmc
