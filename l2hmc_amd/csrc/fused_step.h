// Chain-local and step stages of the whole-step kernels, held ONCE for their three forms (fused_traj.hip: 16 rows per
// workgroup, also ConvNet3D and the taped instances; fused_traj4.hip: 4 / 8 / 12 rows; fused_traj32.hip: 32 rows).
// The forms differ in their product loops and net_update; what surrounds them -- the Philox draws and the staging of
// x and v, the plaquette passes, the accept probability, the mix of the directions with Metropolis-Hastings, the
// observables, the fixed-order step sums and the write-back -- is the same arithmetic in the same order, so the forms
// give the same bits by construction (tests/test_gpu_parity.py::test_subtile_and_32_row_forms_equal_16_row_form).
//
// Template parameters, the same names everywhere: ROWS per workgroup, THREADS of the workgroup, D = x_dim, SX / SP =
// LDS row strides of the x / v / force rows and of the sin P rows, TPC = threads per chain in the chain-local passes,
// NCH = chains one thread group walks per pass (chain ROWS / NCH * h + fc0 for h < NCH), NLD = log-det partial rows
// per chain, TREE = width of the final sum tree.
#pragma once
#include "fused_common.h"
#include "fused_args.h"

namespace l2hmc {

// Per-workgroup scalars of the stages below, and the step-mode scratch in LDS.
struct StepWg {
  int tid;
  int64_t row0;       // trajectory mode: first row of the workgroup
  int nrow;           //   and its live rows
  bool stepm;         // whole-step mode (FusedArgs::step_B > 0)
  bool split;         // split step mode (FusedArgs::step_split): ROWS chains of one direction, uniform over the workgroup
  bool paired;        // ROWS / 2 chains x both directions: rows [0, ROWS / 2) forward, the rest backward
  int sdw;            // (split) this workgroup's direction
  int cpw;            // chains per workgroup in step mode
  int64_t cbase;      //   and its first chain
  float* scoin;       // [ROWS] direction coin per chain slot
  float* su;          // [ROWS] MH uniform
  float* spx;         // [ROWS] accept probability per row
  float* sobs;        // [ROWS][4] sum cos P (in), sum project P (in), sum project P (out), p
  float* sbeta;       // [ROWS] LADDER instances: beta of the chain every row belongs to (stage_chains)
};

// stp: [8 * ROWS] floats of LDS (coin, u, p_row, obs [4], beta).  split: only the 16-row GenericNet sampling instance
// has that layout.
template <int ROWS>
__device__ __forceinline__ StepWg step_workgroup(const FusedArgs& p, float* stp, bool split) {
  StepWg w;
  w.tid = threadIdx.x;
  w.row0 = (int64_t)blockIdx.x * ROWS;
  w.nrow = (int)min((int64_t)ROWS, p.rows - w.row0);
  w.stepm = p.step_B > 0;
  w.split = split;
  w.paired = w.stepm && p.step_both && !split;
  w.sdw = split ? (int)(blockIdx.x & 1) : 0;
  w.cpw = w.paired ? ROWS / 2 : ROWS;
  w.cbase = split ? (int64_t)(blockIdx.x >> 1) * ROWS : (int64_t)blockIdx.x * w.cpw;
  w.scoin = stp;
  w.su = stp + ROWS;
  w.spx = stp + 2 * ROWS;
  w.sobs = stp + 3 * ROWS;
  w.sbeta = stp + 7 * ROWS;
  return w;
}

// element `elem` of l2hmc_fill_uniform's stream
__device__ __forceinline__ float philox_u01(uint64_t seed, uint64_t elem, uint64_t stream) {
  const uint64_t b = elem >> 2;
  uint32_t c[4] = {(uint32_t)b, (uint32_t)(b >> 32), (uint32_t)stream, (uint32_t)(stream >> 32)};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  return (float)(c[elem & 3] >> 8) * (1.0f / 16777216.0f);
}

// ---- stage chain state: x rows -> xs, v rows -> vs, the rows' directions -> sdir [ROWS], their betas -> w.sbeta ---
// Step mode draws the coin and the MH uniform of every chain and the momenta of its rows; trajectory mode reads x0 / v0.
// LADDER (step mode with FusedArgs::step_betas, an instance of its own so that the uniform step stays the code it
// was): the beta of a row is that of the row's CHAIN -- both directions of a chain (paired layout: rows r and
// r + ROWS / 2; split layout: the same row of the pair's two workgroups) run at one value.  A dead row (chain >=
// step_Bl) reads nothing and takes FusedArgs::beta.
// LADDER && TRAJ (the taped forward of a training step on a ladder, trajectory mode, again instances of their own):
// live row r of the launch takes step_betas[(r % step_beta_mod) * step_beta_stride], a dead row FusedArgs::beta -- 0
// in a ladder launch (train.hip passes RowBeta's scalar slot); a dead row holds zeros and is never written back.
template <int ROWS, int THREADS, int D, int SX, bool LADDER = false, bool TRAJ = false>
__device__ __forceinline__ void stage_chains(const FusedArgs& p, const StepWg& w, float* xs, float* vs, int* sdir) {
  const int tid = w.tid;
  if (w.stepm) {
    if (tid < w.cpw) {
      const int64_t chain = w.cbase + tid;
      const bool lv = chain < p.step_Bl;          // (streams are indexed by the chain's place in the WHOLE batch)
      w.scoin[tid] = lv ? philox_u01(p.step_seed, (uint64_t)(p.step_chain0 + chain), 2 * p.step_draw + 1) : 1.f;
      w.su[tid] = lv ? philox_u01(p.step_seed, (uint64_t)(p.step_B + p.step_chain0 + chain), 2 * p.step_draw + 1) : 1.f;
    }
    __syncthreads();
    for (int i = tid; i < ROWS * (D / 4); i += THREADS) {
      const int rr = i / (D / 4), c4 = (i - rr * (D / 4)) * 4;
      const int k = w.paired ? (rr >= ROWS / 2 ? rr - ROWS / 2 : rr) : rr;
      const int64_t chain = w.cbase + k;
      const int dsel = w.split ? w.sdw : w.paired ? (rr >= ROWS / 2 ? 1 : 0) : (w.scoin[k] > 0.5f ? 0 : 1);   // gauge_dynamics.py:221-227
      f32x4 xv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
      if (chain < p.step_Bl) {
        xv = *reinterpret_cast<const f32x4*>(p.x0 + chain * D + c4);
        // momentum of (direction dsel, chain): elements [(dsel * B + chain) * D, + D) of the normal stream
        const uint64_t nb = (((uint64_t)dsel * (uint64_t)p.step_B + (uint64_t)(p.step_chain0 + chain)) * D + c4) >> 2;
        uint32_t c[4] = {(uint32_t)nb, (uint32_t)(nb >> 32), (uint32_t)(2 * p.step_draw), (uint32_t)((2 * p.step_draw) >> 32)};
        philox4x32_10(c, (uint32_t)p.step_seed, (uint32_t)(p.step_seed >> 32));
        float nv[4];
        philox_normal4(c, nv);
        vv = f32x4{nv[0], nv[1], nv[2], nv[3]};
      }
      *reinterpret_cast<f32x4*>(xs + rr * SX + c4) = xv;
      *reinterpret_cast<f32x4*>(vs + rr * SX + c4) = vv;
    }
  } else {
    for (int i = tid; i < ROWS * (D / 4); i += THREADS) {
      const int rr = i / (D / 4), c4 = (i - rr * (D / 4)) * 4;
      f32x4 xv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
      if (rr < w.nrow) {
        const int64_t xr = p.x_mod > 0 ? (w.row0 + rr) % p.x_mod : w.row0 + rr;
        xv = *reinterpret_cast<const f32x4*>(p.x0 + xr * D + c4);
        vv = *reinterpret_cast<const f32x4*>(p.v0 + (w.row0 + rr) * D + c4);
      }
      *reinterpret_cast<f32x4*>(xs + rr * SX + c4) = xv;
      *reinterpret_cast<f32x4*>(vs + rr * SX + c4) = vv;
    }
  }
  if (tid < ROWS) {
    int d = 0;
    if (w.stepm) d = w.split ? w.sdw : w.paired ? (tid >= ROWS / 2 ? 1 : 0) : (w.scoin[tid] > 0.5f ? 0 : 1);
    else if (tid < w.nrow) d = p.dir ? p.dir[w.row0 + tid] : (p.dir_split > 0 && w.row0 + tid >= p.dir_split) ? 1 : 0;
    sdir[tid] = d;
    if constexpr (LADDER && TRAJ) {
      w.sbeta[tid] = tid < w.nrow ? p.step_betas[((w.row0 + tid) % p.step_beta_mod) * p.step_beta_stride] : p.beta;
    } else if constexpr (LADDER) {
      const int64_t chain = w.cbase + (w.paired && tid >= ROWS / 2 ? tid - ROWS / 2 : tid);
      w.sbeta[tid] = chain < p.step_Bl ? p.step_betas[chain * p.step_beta_stride] : p.beta;
    }
  }
}

// per-net constants kept in LDS: b1[H] wt[2H] bh[H] bhd[3D] exp(cs)[D] exp(cq)[D]
template <int THREADS, int D, int H>
__device__ __forceinline__ void load_consts(const l2hmc_dense_net& n, float* c, int tid) {
  for (int i = tid; i < H; i += THREADS) {
    c[i] = n.b1[i];
    c[H + i] = n.wt[i];
    c[2 * H + i] = n.wt[H + i];
    c[3 * H + i] = n.bh[i];
  }
  for (int i = tid; i < 3 * D; i += THREADS) c[4 * H + i] = n.bhd[i];
  for (int i = tid; i < D; i += THREADS) {
    c[4 * H + 3 * D + i] = expf(n.coeff_s[i]);
    c[4 * H + 4 * D + i] = expf(n.coeff_q[i]);
  }
}

// ---- chain-local passes: TPC consecutive threads per chain ------------------------------------------------------
// The terms of a chain are strided by TPC and summed by a butterfly over TPC lanes; these sums are part of the
// result's bits, so every GenericNet form keeps TPC = 16 whatever its rows and wave count.  A thread group walks NCH
// chains per pass (chain ROWS / NCH * h + fc0); the threads beyond ROWS / NCH x TPC walk empty loops (their fl lies
// beyond every loop bound) and take part in the barriers only.
struct ChainLanes {
  int fc0, fl;           // chain (of pass 0), lane-in-chain; fl = kIdleLane for a thread without a chain
  int T, X, xsh;         // sites = 64 and X divides it: shifts instead of run-time divisions
  float beta;
  const float* sbeta;    // LADDER instances: StepWg::sbeta, beta per row (LDS), read where it is used
};

constexpr int kIdleLane = 1 << 20;

template <int ROWS, int TPC, int NCH>
__device__ __forceinline__ ChainLanes chain_lanes(const FusedArgs& p, const StepWg& w, int tid) {
  ChainLanes c;
  const bool own = tid < ROWS / NCH * TPC;
  c.fc0 = own ? tid / TPC : 0;
  c.fl = own ? tid % TPC : kIdleLane;
  c.T = p.T;
  c.X = p.X;
  c.xsh = 31 - __clz(p.X);
  c.beta = p.beta;
  c.sbeta = w.sbeta;
  return c;
}

template <int TPC>
__device__ __forceinline__ float chain_sum(float v) {
#pragma unroll
  for (int off = TPC / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// force (beta * dS/dx) of the x rows into gs; act[h] = the action of chain ROWS / NCH * h + fc0 (all TPC lanes of the
// chain).  One barrier between the sin P pass and the force pass for all NCH chains, one behind the force pass.
template <int ROWS, int TPC, int NCH, int D, int SX, int SP, bool LADDER = false>
__device__ __forceinline__ void force_pass(const ChainLanes& c, const float* xs, float* sp, float* gs, float (&act)[NCH]) {
  constexpr int sites = D / 2;
  const int T = c.T, X = c.X, xsh = c.xsh;
#pragma unroll
  for (int h = 0; h < NCH; ++h) {
    const int fc = ROWS / NCH * h + c.fc0;
    const float* xc = xs + fc * SX;
    float a = 0.f;
    for (int s = c.fl; s < sites; s += TPC) {
      const int i = s >> xsh, j = s & (X - 1);            // X is a power of two (T * X = 64)
      const int jp = (j + 1 == X) ? 0 : j + 1, ip = (i + 1 == T) ? 0 : i + 1;
      const float P = xc[2 * s] - xc[2 * s + 1] - xc[2 * (i * X + jp)] + xc[2 * (ip * X + j) + 1];
      float sn, cs;
      fast_sincos(P, &sn, &cs);
      sp[fc * SP + s] = sn;
      a += 1.f - cs;
    }
    act[h] = chain_sum<TPC>(a);
  }
  __syncthreads();
#pragma unroll
  for (int h = 0; h < NCH; ++h) {
    const int fc = ROWS / NCH * h + c.fc0;
    float* gc = gs + fc * SX;
    const float* spc = sp + fc * SP;
    const float beta = LADDER ? c.sbeta[fc] : c.beta;
    for (int s = c.fl; s < sites; s += TPC) {
      const int i = s >> xsh, j = s & (X - 1);            // X is a power of two (T * X = 64)
      const int jm = (j == 0) ? X - 1 : j - 1, im = (i == 0) ? T - 1 : i - 1;
      const float sP = spc[s];
      gc[2 * s] = beta * (sP - spc[i * X + jm]);
      gc[2 * s + 1] = beta * (-sP + spc[im * X + j]);
    }
  }
  __syncthreads();
}

template <int ROWS, int TPC, int NCH, int D, int SX>
__device__ __forceinline__ void kinetic_pass(const ChainLanes& c, const float* vs, float (&kin)[NCH]) {
#pragma unroll
  for (int h = 0; h < NCH; ++h) {
    const float* vc = vs + (ROWS / NCH * h + c.fc0) * SX;
    float k = 0.f;
    for (int d = c.fl; d < D; d += TPC) k += vc[d] * vc[d];
    kin[h] = 0.5f * chain_sum<TPC>(k);
  }
}

// sum cos P and sum of P projected to [-pi, pi) over the plaquettes of the chain at xc
template <int TPC, int D>
__device__ __forceinline__ void plaq_sums(const ChainLanes& c, const float* xc, float& scos, float& sproj) {
  const int T = c.T, X = c.X, xsh = c.xsh;
  const float inv2pi = 0.15915494309189533577f;
  float a = 0.f, b = 0.f;
  for (int st = c.fl; st < D / 2; st += TPC) {
    const int i = st >> xsh, j = st & (X - 1);
    const int jp = (j + 1 == X) ? 0 : j + 1, ip = (i + 1 == T) ? 0 : i + 1;
    const float P = xc[2 * st] - xc[2 * st + 1] - xc[2 * (i * X + jp)] + xc[2 * (ip * X + j) + 1];
    float sn, cs;
    fast_sincos(P, &sn, &cs);
    a += cs;
    b += P - 6.28318530717958647692f * floorf((P + 3.14159265358979323846f) * inv2pi);   // project_angle
  }
  scos = chain_sum<TPC>(a);
  sproj = chain_sum<TPC>(b);
}

// ---- accept probability ------------------------------------------------------------------------------------------
// log-det of row fc: its NLD partial sums in ldw [NLD][ROWS] (fixed order: bit-reproducible)
template <int ROWS, int NLD>
__device__ __forceinline__ float sum_logdet(const float* ldw, int fc) {
  float sld = 0.f;
#pragma unroll
  for (int w = 0; w < NLD; ++w) sld += ldw[w * ROWS + fc];
  return sld;
}

// gauge_dynamics.py:592-609; the O(100) Hamiltonians are differenced in fp64
__device__ __forceinline__ float accept_prob(float beta, float act0, float act1, float kin0, float kin1, float sld) {
  const double dh = (double)beta * ((double)act0 - (double)act1) + ((double)kin0 - (double)kin1) + (double)sld;
  return accept_from_delta(dh);
}

// step mode: the accept probability of every row -> spx (the caller's barrier follows)
template <int ROWS, int NCH, int NLD, bool LADDER = false>
__device__ __forceinline__ void step_accept_probs(const ChainLanes& c, const float* ldw, const float (&act0)[NCH],
                                                  const float (&act1)[NCH], const float (&kin0)[NCH],
                                                  const float (&kin1)[NCH], float* spx) {
  if (c.fl == 0) {
#pragma unroll
    for (int h = 0; h < NCH; ++h) {
      const int fc = ROWS / NCH * h + c.fc0;
      const float beta = LADDER ? c.sbeta[fc] : c.beta;
      spx[fc] = accept_prob(beta, act0[h], act1[h], kin0[h], kin1[h], sum_logdet<ROWS, NLD>(ldw, fc));
    }
  }
}

// trajectory mode: log-det and accept probability of the live rows
template <int ROWS, int NCH, int NLD, bool LADDER = false>
__device__ __forceinline__ void traj_logdet_accept(const FusedArgs& p, const StepWg& w, const ChainLanes& c,
                                                   const float* ldw, const float (&act0)[NCH], const float (&act1)[NCH],
                                                   const float (&kin0)[NCH], const float (&kin1)[NCH]) {
  if (c.fl == 0) {
#pragma unroll
    for (int h = 0; h < NCH; ++h) {
      const int fc = ROWS / NCH * h + c.fc0;
      if (fc < w.nrow) {
        const float sld = sum_logdet<ROWS, NLD>(ldw, fc);
        const int64_t rr = w.row0 + fc;
        if (p.logdet) p.logdet[rr] = p.logdet_accumulate ? p.logdet[rr] + sld : sld;
        const float beta = LADDER ? c.sbeta[fc] : c.beta;
        if (p.p_accept) p.p_accept[rr] = accept_prob(beta, act0[h], act1[h], kin0[h], kin1[h], sld);
      }
    }
  }
}

// trajectory mode: the live rows of xs / vs -> x_out / v_out
template <int ROWS, int THREADS, int D, int SX>
__device__ __forceinline__ void traj_write_back(const FusedArgs& p, const StepWg& w, const float* xs, const float* vs) {
  for (int i = w.tid; i < ROWS * (D / 4); i += THREADS) {
    const int rr = i / (D / 4), c4 = (i - rr * (D / 4)) * 4;
    if (rr < w.nrow) {
      *reinterpret_cast<f32x4*>(p.x_out + (w.row0 + rr) * D + c4) = *reinterpret_cast<const f32x4*>(xs + rr * SX + c4);
      *reinterpret_cast<f32x4*>(p.v_out + (w.row0 + rr) * D + c4) = *reinterpret_cast<const f32x4*>(vs + rr * SX + c4);
    }
  }
}

// ---- step mode: mix the two directions, Metropolis-Hastings (gauge_dynamics.py:221-257, arithmetic kept as
//      mask * a + (1 - mask) * b); x_in -> gin rows, x_out -> gout rows (LDS the caller has free, stride SX).
// xfr / xbr, vfr / vbr: forward / backward rows of chain k (stride SX), pfr / pbr their accept probabilities; with
// step_both = 0 the chain's one row and probability are the "forward" ones.
template <int THREADS, int D, int SX>
__device__ __forceinline__ void step_mix_accept(const FusedArgs& p, const StepWg& w, const float* xfr, const float* xbr,
                                                const float* vfr, const float* vbr, const float* pfr, const float* pbr,
                                                float* gin, float* gout) {
  for (int i = w.tid; i < w.cpw * (D / 4); i += THREADS) {
    const int k = i / (D / 4), c4 = (i - k * (D / 4)) * 4;
    const int64_t chain = w.cbase + k;
    f32x4 xin = {0.f, 0.f, 0.f, 0.f};
    if (chain < p.step_Bl) xin = *reinterpret_cast<const f32x4*>(p.x0 + chain * D + c4);
    f32x4 xp;
    float pk;
    if (p.step_both) {
      const float fm = w.scoin[k] > 0.5f ? 1.f : 0.f, bm = 1.f - fm;
      pk = fm * pfr[k] + bm * pbr[k];
      const f32x4 xf = *reinterpret_cast<const f32x4*>(xfr + k * SX + c4);
      const f32x4 xb = *reinterpret_cast<const f32x4*>(xbr + k * SX + c4);
      xp = fm * xf + bm * xb;
    } else {
      pk = pfr[k];
      xp = *reinterpret_cast<const f32x4*>(xfr + k * SX + c4);
    }
    const float am = pk > w.su[k] ? 1.f : 0.f;                       // strict >, quirk Q5
    const f32x4 xo = am * xp + (1.f - am) * xin;
    *reinterpret_cast<f32x4*>(gin + k * SX + c4) = xin;
    *reinterpret_cast<f32x4*>(gout + k * SX + c4) = xo;
    if (c4 == 0) w.sobs[k * 4 + 3] = pk;
    if (chain < p.step_Bl) {                                       // apply_transition's own outputs (:259)
      if (p.step_xprop) *reinterpret_cast<f32x4*>(p.step_xprop + chain * D + c4) = xp;
      if (p.step_xout) *reinterpret_cast<f32x4*>(p.step_xout + chain * D + c4) = xo;
      if (p.step_vprop) {
        f32x4 vp = *reinterpret_cast<const f32x4*>(vfr + k * SX + c4);
        if (p.step_both) {
          const float fm = w.scoin[k] > 0.5f ? 1.f : 0.f, bm = 1.f - fm;
          vp = fm * vp + bm * *reinterpret_cast<const f32x4*>(vbr + k * SX + c4);
        }
        *reinterpret_cast<f32x4*>(p.step_vprop + chain * D + c4) = vp;
      }
    }
  }
  __syncthreads();
}

// ---- step mode: observables of the step's INPUT samples (gauge_model.py:256-266) and the charge of its output
//      (:718-725), then the per-chain outputs.  Paired layout: thread group fc measures gin of chain fc, or gout of
//      chain fc - ROWS / 2; otherwise both of chain fc.
template <int ROWS, int TPC, int NCH, int D, int SX>
__device__ __forceinline__ void step_observables(const FusedArgs& p, const StepWg& w, const ChainLanes& c,
                                                 const float* gin, const float* gout) {
  constexpr int sites = D / 2;
  float* sobs = w.sobs;
#pragma unroll
  for (int h = 0; h < NCH; ++h) {
    const int fc = ROWS / NCH * h + c.fc0;
    if (w.paired) {
      float a, b;
      plaq_sums<TPC, D>(c, fc < ROWS / 2 ? gin + fc * SX : gout + (fc - ROWS / 2) * SX, a, b);
      if (c.fl == 0) {
        if (fc < ROWS / 2) { sobs[fc * 4 + 0] = a; sobs[fc * 4 + 1] = b; }
        else sobs[(fc - ROWS / 2) * 4 + 2] = b;
      }
    } else {
      float a, b, c_, d_;
      plaq_sums<TPC, D>(c, gin + fc * SX, a, b);
      plaq_sums<TPC, D>(c, gout + fc * SX, c_, d_);
      if (c.fl == 0) { sobs[fc * 4 + 0] = a; sobs[fc * 4 + 1] = b; sobs[fc * 4 + 2] = d_; }
    }
  }
  __syncthreads();
  const float inv2pi = 0.15915494309189533577f;
  if (w.tid < w.cpw) {
    const int64_t chain = w.cbase + w.tid;
    if (chain < p.step_Bl) {
      const float q_in = sobs[w.tid * 4 + 1] * inv2pi, q_out = sobs[w.tid * 4 + 2] * inv2pi;
      if (p.step_px) p.step_px[chain] = sobs[w.tid * 4 + 3];
      if (p.step_act) p.step_act[chain] = (float)sites - sobs[w.tid * 4 + 0];      // sum (1 - cos P)
      if (p.step_plq) p.step_plq[chain] = sobs[w.tid * 4 + 0] / (float)sites;
      if (p.step_chg) p.step_chg[chain] = q_in;
      if (p.step_dq) p.step_dq[chain] = fabsf(q_in - q_out);
    }
  }
}

// ---- step mode: [sum p_accept, sum |dQ|, chains] in a fixed order and without a further launch: every workgroup
//      leaves its partial sums in step_part, the last one to arrive (ticket in step_sums[3]) adds them up and resets
//      the ticket.  A workgroup fills ngrp slots from slot0 on, one per cpw / ngrp of its chains; npart slots are
//      summed by the last of nfin finishers over a tree of TREE threads (TREE is part of the sums' bits).
//      fin: [2][TREE] floats of LDS the caller has free.
template <int THREADS, int TREE>
__device__ __forceinline__ void step_sums(const FusedArgs& p, const StepWg& w, int ngrp, int64_t slot0, int npart,
                                          int nfin, float* fin) {
  if (!p.step_sums) return;
  const int tid = w.tid;
  const float inv2pi = 0.15915494309189533577f;
  const float* sobs = w.sobs;
  int* last = reinterpret_cast<int*>(w.spx);            // spx is free again
  const int gch = w.cpw / ngrp;
  if (tid == 0) {
    for (int g = 0; g < ngrp; ++g) {
      float a0 = 0.f, a1 = 0.f;
      for (int k = g * gch; k < (g + 1) * gch; ++k) {
        if (w.cbase + k < p.step_Bl) {
          a0 += sobs[k * 4 + 3];
          a1 += fabsf(sobs[k * 4 + 1] * inv2pi - sobs[k * 4 + 2] * inv2pi);
        }
      }
      if (slot0 + g < npart) {
        p.step_part[2 * (slot0 + g)] = a0;
        p.step_part[2 * (slot0 + g) + 1] = a1;
      }
    }
    __threadfence();
    *last = atomicAdd(reinterpret_cast<int*>(p.step_sums + 3), 1) == nfin - 1;
  }
  __syncthreads();
  if (*last) {
    __threadfence();
    const bool leaf = THREADS == TREE || tid < TREE;    // (TREE partial sums and their tree, whatever the thread count)
    float a0 = 0.f, a1 = 0.f;
    for (int b = tid; leaf && b < npart; b += TREE) {
      a0 += p.step_part[2 * b];
      a1 += p.step_part[2 * b + 1];
    }
    if (leaf) {
      fin[tid] = a0;
      fin[TREE + tid] = a1;
    }
    __syncthreads();
    for (int st = TREE / 2; st > 0; st >>= 1) {
      if (tid < st) {
        fin[tid] += fin[tid + st];
        fin[TREE + tid] += fin[TREE + tid + st];
      }
      __syncthreads();
    }
    if (tid == 0) {
      p.step_sums[0] = p.step_sums_acc ? p.step_sums[0] + fin[0] : fin[0];          // (a batch cut into two launches)
      p.step_sums[1] = p.step_sums_acc ? p.step_sums[1] + fin[TREE] : fin[TREE];
      p.step_sums[2] = (float)p.step_B;
      *reinterpret_cast<int*>(p.step_sums + 3) = 0;
    }
  }
}

// ---- step mode: np.mod(x_out, 2 pi) (gauge_model.py:1388) and the write-back of the chains' new state
template <int THREADS, int D, int SX>
__device__ __forceinline__ void step_write_next(const FusedArgs& p, const StepWg& w, const float* gout) {
  for (int i = w.tid; p.step_x_next && i < w.cpw * (D / 4); i += THREADS) {
    const int k = i / (D / 4), c4 = (i - k * (D / 4)) * 4;
    const int64_t chain = w.cbase + k;
    if (chain < p.step_Bl) {
      f32x4 wv = *reinterpret_cast<const f32x4*>(gout + k * SX + c4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float tp = 6.28318530717958647692f;
        float m_ = fmaf(-tp, floorf(wv[e] * 0.15915494309189533577f), wv[e]);       // w - 2 pi floor(w / 2 pi)
        if (m_ < 0.f) m_ += tp;
        if (m_ >= tp) m_ -= tp;
        wv[e] = m_;
      }
      *reinterpret_cast<f32x4*>(p.step_x_next + chain * D + c4) = wv;
    }
  }
}

}  // namespace l2hmc
