// Plain HMC on the 2D U(1) lattice in ONE launch, at a lattice size chosen at run time: the whole MCMC step
// (l2hmc_gauge_mcmc_step, l2hmc_gauge_transition_draw) or a whole trajectory / single leapfrog step
// (l2hmc_gauge_trajectory, l2hmc_gauge_leapfrog) of plans with hmc = 1 (gauge_dynamics.py:102-108: S = T = Q = 0), and
// a whole RUN of MCMC steps in one launch (l2hmc_gauge_hmc_run: hmc_run_kernel loops over the one copy of the step;
// l2hmc_gauge_hmc_run_ladder: the same run with beta and the step size per chain; l2hmc_gauge_hmc_run_exchange: the
// ladder run with the replica-exchange rounds inside the launch, hmc_run_exchange_kernel, a workgroup per replica group).
//
// Without networks a leapfrog step is a few flops and ONE sin per plaquette, so the kernel is transcendental- and
// latency-bound and its mapping is chosen for waves in flight, not for the matrix pipe:
//   * a ROW (chain x direction) is walked by TPC = 2^k threads, thread fl owning the SPT sites fl, fl + TPC, ...
//     (SPT = 1 up to 256 sites, 2 up to 512, 4 up to 1024): both links of its sites and their momenta stay in
//     REGISTERS for the whole trajectory.  The momentum and position sub-updates are link-local and never leave them;
//   * LDS holds a row's x as two planes [2][sites] (for the two neighbour links a plaquette needs: consecutive lanes
//     read consecutive words, no bank conflict) and sin P (for the two neighbour plaquettes a link's force needs).
//     The force itself is never stored: the momentum half-kick forms it from sin P.  Two barriers per leapfrog step
//     (x published, sin P published);
//   * a workgroup of 256 threads (512 where TPC = 256) holds 256 / TPC rows: 32 rows of a 2 x 4 lattice, 2 of a
//     32 x 32 one.  In step mode with both directions they are the forward and the backward rows of the same chains
//     (rows [0, R / 2) forward), so mixing, Metropolis-Hastings and the observables need no other workgroup.
// The force at the end of a step is the force at the start of the next (x has not moved): one sin P pass per leapfrog
// step plus one, against two in the layered path -- the same values, kept.
//
// Arithmetic: the sub-updates are those of lf_update_v_kernel / lf_update_x_kernel with S = T = Q = 0 (exp(0) = 1
// folded), masks and step index num_steps - 1 - step for backward rows, two masked position sub-updates per step;
// sin / cos are fast_sincos (u1_lattice.hip's).  The Philox draws, the fp64 accept probability, the fixed-order step
// sums and the wrap are fused_step.h's own code.  The per-row sums (action, kinetic energy, sum cos P, sum project P)
// are grouped differently from fused_step.h's 16-lane form: a thread adds its SPT terms in ascending order, a
// butterfly adds the threads of a wave, waves are added in ascending order.
#include <type_traits>

#include "gauge_swap.h"

namespace l2hmc {

constexpr int kHmcMaxSites = 1024;        // 4 sites per thread x 256 threads per row
constexpr int kHmcMaxThreads = 512;

struct HmcGeom {
  int spt, tsh, threads, rows_wg;         // sites per thread, log2(threads per row), workgroup size, rows per workgroup
  size_t lds;
};

// floats per row that the ladder run of `spt` sites per thread keeps in LDS on top of HmcGeom::lds (HmcRowLds)
constexpr int hmc_ladder_lds_floats(int spt) { return spt == 4 ? 2 : 0; }

static bool hmc_geom(int T, int X, HmcGeom* g) {
  if (T <= 0 || X <= 0 || (int64_t)T * X > kHmcMaxSites) return false;
  const int sites = T * X;
  g->spt = sites <= 256 ? 1 : sites <= 512 ? 2 : 4;
  const int per = (sites + g->spt - 1) / g->spt;
  g->tsh = 0;
  while ((1 << g->tsh) < per) ++g->tsh;
  g->threads = g->tsh == 8 ? kHmcMaxThreads : 256;
  g->rows_wg = g->threads >> g->tsh;
  // xs, vs [R][D], sin P [R][sites], step scratch [8 R], wave partials [R][4][2], sum tree [2][256]: 42 KiB at most
  g->lds = sizeof(float) * ((size_t)g->rows_wg * (5 * sites + 8 + 8) + 2 * 256);
  return true;
}

int hmc_plan_supported(const l2hmc_gauge_plan* p) {
  HmcGeom g;
  return p->hmc && p->num_steps > 0 && hmc_geom(p->T, p->X, &g);
}

// sums a and b over the threads of a row; every thread of the workgroup calls it (barriers where a row spans waves)
__device__ __forceinline__ void hmc_row_sum2(float& a, float& b, int tsh, int r, int fl, float* red) {
  const int w = tsh < 6 ? 1 << tsh : 64;
  for (int off = w >> 1; off > 0; off >>= 1) {
    a += __shfl_xor(a, off, 64);
    b += __shfl_xor(b, off, 64);
  }
  if (tsh > 6) {
    const int nw = 1 << (tsh - 6);
    if ((fl & 63) == 0) {
      red[(r * 4 + (fl >> 6)) * 2] = a;
      red[(r * 4 + (fl >> 6)) * 2 + 1] = b;
    }
    __syncthreads();
    a = 0.f;
    b = 0.f;
    for (int q = 0; q < nw; ++q) {
      a += red[(r * 4 + q) * 2];
      b += red[(r * 4 + q) * 2 + 1];
    }
    __syncthreads();
  }
}

// What a thread keeps for a whole launch: its place in the workgroup, the carve-up of LDS, its SPT sites and their
// plaquette neighbours.  Nothing of it depends on the MCMC step, so the run kernel forms it once ahead of its step loop.
template <int SPT>
struct HmcLanes {
  int T, X, sites, D, tsh, tpc, R, r, fl;
  float* xs;                                // [R][2][sites]: the x0 links of a row, then its x1 links
  float* vs;                                // [R][2][sites] (step epilogue only)
  float* sp;                                // [R][sites]  sin P
  float* stp;                               // [8 R]       StepWg scratch (+ [R][2] beta, eps in the SPT 4 ladder run)
  float* red;                               // [R][4][2]   per-wave partial sums of a row
  float* fin;                               // [2][256]
  float* xrow;                              // the thread's row of xs
  float* sprow;                             //   and of sp
  bool ok[SPT];
  int nr[SPT], nu[SPT], nl[SPT], nd[SPT];
};

// stp_extra: floats per row that the launch adds to the step scratch (hmc_ladder_lds_floats; 0 for every other launch)
template <int SPT>
__device__ __forceinline__ HmcLanes<SPT> hmc_lanes(const FusedArgs& p, int tsh, float* lds, int tid,
                                                   const int stp_extra = 0) {
  HmcLanes<SPT> g;
  g.T = p.T;
  g.X = p.X;
  g.sites = p.T * p.X;
  g.D = 2 * g.sites;
  g.tsh = tsh;
  g.tpc = 1 << tsh;
  g.R = (int)blockDim.x >> tsh;
  g.r = tid >> tsh;
  g.fl = tid & (g.tpc - 1);
  g.xs = lds;
  g.vs = g.xs + g.R * g.D;
  g.sp = g.vs + g.R * g.D;
  g.stp = g.sp + g.R * g.sites;
  g.red = g.stp + (8 + stp_extra) * g.R;
  g.fin = g.red + 8 * g.R;
  g.xrow = g.xs + g.r * g.D;
  g.sprow = g.sp + g.r * g.sites;
  const int T = g.T, X = g.X;
#pragma unroll
  for (int j = 0; j < SPT; ++j) {
    const int s = g.fl + j * g.tpc;
    g.ok[j] = s < g.sites;
    const int sc = g.ok[j] ? s : 0;
    const int i = sc / X, jx = sc - i * X;
    g.nr[j] = i * X + (jx + 1 == X ? 0 : jx + 1);
    g.nl[j] = i * X + (jx == 0 ? X - 1 : jx - 1);
    g.nu[j] = (i + 1 == T ? 0 : i + 1) * X + jx;
    g.nd[j] = (i == 0 ? T - 1 : i - 1) * X + jx;
  }
  return g;
}

template <int SPT>
__device__ __forceinline__ StepWg hmc_workgroup(const FusedArgs& p, const HmcLanes<SPT>& g) {
  const int R = g.R;
  StepWg w;
  w.tid = threadIdx.x;
  w.row0 = (int64_t)blockIdx.x * R;
  w.nrow = (int)min((int64_t)R, p.rows - w.row0);
  w.stepm = p.step_B > 0;
  w.split = false;
  w.paired = w.stepm && p.step_both;
  w.sdw = 0;
  w.cpw = w.paired ? R / 2 : R;
  w.cbase = (int64_t)blockIdx.x * w.cpw;
  w.scoin = g.stp;
  w.su = g.stp + R;
  w.spx = g.stp + 2 * R;
  w.sobs = g.stp + 3 * R;
  w.sbeta = nullptr;                      // (unused: hmc_step takes the row's beta as an argument)
  return w;
}

// beta and the step size of a ROW, as the trajectory takes them.  HmcRowValues: two values (the step and trajectory
// kernels and the uniform run pass p.beta and p.eps, uniform over the launch; the ladder run of SPT 1 and 2 the pair of
// the row's chain, in two registers).  HmcRowLds: the pair in the row's LDS scratch, read where it is used, so that it
// is live in no register across the trajectory (the ladder run of SPT 4, which has no register to spare).
struct HmcRowValues {
  float b, e;
  __device__ __forceinline__ float beta() const { return b; }
  __device__ __forceinline__ float eps() const { return e; }
};
struct HmcRowLds {
  const float* be;                          // [beta, eps] of the row
  __device__ __forceinline__ float beta() const { return be[0]; }
  __device__ __forceinline__ float eps() const { return be[1]; }
};

// The trajectory of the thread's row from (x, v) in registers, direction d (0 forward, 1 backward), steps
// [p.step_begin, p.step_end) at the ROW's beta with the row's step size (be; p.beta and p.eps are not read); returns
// the row's accept probability (0 unless want_p).  Every thread of the workgroup calls it.  On return the row's x is
// also in its xs row (published ahead of the last sin P pass).
// HOLD_LDS: where the thread's shares of the action and the kinetic energy at the start wait for the end (see below).
template <int SPT, bool HOLD_LDS, class BE>
__device__ __forceinline__ float hmc_trajectory(const FusedArgs& p, const HmcLanes<SPT>& g, const BE be, const int d,
                                                const bool want_p, float (&x0)[SPT], float (&x1)[SPT],
                                                float (&v0)[SPT], float (&v1)[SPT]) {
  const int sites = g.sites, D = g.D, tpc = g.tpc, fl = g.fl;
  float* xrow = g.xrow;
  float* sprow = g.sprow;
  float sP[SPT];

  auto publish_x = [&]() {
#pragma unroll
    for (int j = 0; j < SPT; ++j)
      if (g.ok[j]) {
        xrow[fl + j * tpc] = x0[j];
        xrow[sites + fl + j * tpc] = x1[j];
      }
    __syncthreads();
  };
  // sin P of the thread's sites -> sP and LDS; returns the thread's share of the action sum (1 - cos P)
  auto sin_pass = [&]() {
    float a = 0.f;
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      sP[j] = 0.f;
      if (g.ok[j]) {
        // gauge_model.py:676-679: x0[i,j] - x1[i,j] - x0[i,j+1] + x1[i+1,j]
        const float P = x0[j] - x1[j] - xrow[g.nr[j]] + xrow[sites + g.nu[j]];
        float sn, cs;
        fast_sincos(P, &sn, &cs);
        sP[j] = sn;
        sprow[fl + j * tpc] = sn;
        a += 1.f - cs;
      }
    }
    __syncthreads();
    return a;
  };
  // momentum half-kick (lf_update_v_kernel with S = T = Q = 0): force = beta dS/dx from sin P
  auto kick = [&]() {
    const float beta = be.beta(), eps = be.eps();
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      if (g.ok[j]) {
        const float g0 = beta * (sP[j] - sprow[g.nl[j]]);
        const float g1 = beta * (-sP[j] + sprow[g.nd[j]]);
        const float k0 = 0.5f * eps * g0, k1 = 0.5f * eps * g1;
        v0[j] = d ? v0[j] + k0 : v0[j] - k0;
        v1[j] = d ? v1[j] + k1 : v1[j] - k1;
      }
    }
  };
  auto kinetic = [&]() {
    float kk = 0.f;
#pragma unroll
    for (int j = 0; j < SPT; ++j) kk += v0[j] * v0[j] + v1[j] * v1[j];
    return kk;
  };

  publish_x();
  // The Hamiltonian difference is summed over the row as the DIFFERENCES of the threads' own shares of the action and
  // of the kinetic energy at the two ends (O(dH) in all), not as totals of O(sites) that are subtracted afterwards: an
  // fp32 total of 1000 carries 6e-5 of rounding, and p = exp(dH) takes all of it once p lies inside (0, 1); a thread's
  // share is of O(10), its rounding 5e-7.  The row is summed once, not twice.
  // The shares at the start wait (HOLD_LDS) in the thread's own two words of the row's v planes, which nobody reads or
  // writes before the step's epilogue (whose last read of them lies behind a barrier); a lane without a first site has
  // no site at all, and its shares are 0.  Only the run kernels of four sites per thread keep them in the two
  // registers that held the totals: with the pair in LDS they take 130 VGPRs and lose their second workgroup per CU
  // (with the pair in registers the step kernel of two sites per thread takes 81 and loses its third; hipcc of ROCm
  // 7.2.0 at -O3).  The values are the same either way.
  float* hold = g.vs + g.r * D + fl;
  const float act0 = sin_pass(), kin0 = want_p ? kinetic() : 0.f;
  if (HOLD_LDS && want_p && g.ok[0]) {
    hold[0] = act0;
    hold[sites] = kin0;
  }
  float act1 = act0;
  const int N = p.num_steps;
  for (int step = p.step_begin; step < p.step_end; ++step) {
    const float* m = p.masks + (size_t)(d ? N - 1 - step : step) * D;     // gauge_dynamics.py:453-457
    float m0[SPT], m1[SPT];
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      const int s = g.ok[j] ? fl + j * tpc : 0;
      m0[j] = m[2 * s];
      m1[j] = m[2 * s + 1];
    }
    kick();
    // two masked position sub-updates (lf_update_x_kernel with S = T = Q = 0): forward keeps m, then 1 - m;
    // backward 1 - m, then m
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      const bool inv = (sub == 1) != (d != 0);
      const float eps = be.eps();
#pragma unroll
      for (int j = 0; j < SPT; ++j) {
        const float ka = inv ? 1.f - m0[j] : m0[j], kb = inv ? 1.f - m1[j] : m1[j];
        const float da = eps * v0[j], db = eps * v1[j];
        const float ua = d ? x0[j] - da : x0[j] + da, ub = d ? x1[j] - db : x1[j] + db;
        x0[j] = ka * x0[j] + (1.f - ka) * ua;
        x1[j] = kb * x1[j] + (1.f - kb) * ub;
      }
    }
    publish_x();
    act1 = sin_pass();
    kick();
  }
  float pr = 0.f;
  if (want_p) {
    float dact = act1, dkin = kinetic();
    if (HOLD_LDS) {
      if (g.ok[0]) {
        dact -= hold[0];
        dkin -= hold[sites];
      }
    } else {
      dact -= act0;
      dkin -= kin0;
    }
    hmc_row_sum2(dact, dkin, g.tsh, g.r, fl, g.red);
    pr = accept_prob(be.beta(), 0.f, dact, 0.f, 0.5f * dkin, 0.f);         // H(start) - H(end) = -(beta dS + dK)
  }
  return pr;
}

// The chain slot and the chain of the thread's row in step mode (they do not change from step to step); a row of
// the paired layout keeps its direction too.
template <int SPT>
__device__ __forceinline__ void hmc_step_row(const FusedArgs& p, const HmcLanes<SPT>& g, const StepWg& w, int& k,
                                             int64_t& grow, bool& live) {
  k = w.paired && g.r >= w.cpw ? g.r - w.cpw : g.r;
  grow = w.cbase + k;
  live = grow < p.step_Bl;
}

// x of chain `grow` -> the thread's registers (zeros for a dead row and for sites beyond the lattice)
template <int SPT>
__device__ __forceinline__ void hmc_load_x(const FusedArgs& p, const HmcLanes<SPT>& g, int64_t grow, bool live,
                                           float (&x0)[SPT], float (&x1)[SPT]) {
#pragma unroll
  for (int j = 0; j < SPT; ++j) {
    x0[j] = x1[j] = 0.f;
    if (g.ok[j] && live) {
      const float* xr = p.x0 + grow * g.D + 2 * (g.fl + j * g.tpc);
      x0[j] = xr[0];
      x1[j] = xr[1];
    }
  }
}

// ONE MCMC step, the only copy (hmc_step_kernel runs it once, hmc_run_kernel once per step of its loop): the coin /
// MH uniform / momentum draws of draw index p.step_draw, the trajectory at be's beta and eps with its fp64 accept
// probability, the mix of the directions with Metropolis-Hastings, the observables of the step's input, |dQ|, the
// wrap and the step's sums.
// In: x0 / x1 = the step's input x of the row's chain (every row, whatever its direction).  Out, in the
// threads of the chains' primary rows (r < w.cpw): x0 / x1 = the wrapped output, the very fp32 values that go to
// p.step_x_next; the other rows' x0 / x1 are left over from their trajectory.  Every per-step pointer of p (step_px
// ... step_dq, step_x_next, step_xprop / _vprop / _xout, step_sums, step_part) is that of THIS step.  p.x0 is not read.
// ngrp, npart: the workgroup fills ngrp slots of the step's npart partial sums (fused_step.h: step_sums), one per
// w.cpw / ngrp of its chains: 1 and the grid size everywhere but in hmc_run_exchange_kernel, whose workgroup holds the
// chains of ngrp workgroups of the ladder run and leaves the partial sums those would.
template <int SPT, bool HOLD_LDS, class BE>
__device__ __forceinline__ void hmc_step(const FusedArgs& p, const HmcLanes<SPT>& g, const StepWg& w, const BE be,
                                         const int k, const int64_t grow, const bool live, float (&x0)[SPT],
                                         float (&x1)[SPT], const int ngrp, const int npart) {
  const int sites = g.sites, D = g.D, tpc = g.tpc, r = g.r, fl = g.fl, tid = w.tid, tsh = g.tsh;
  float* xs = g.xs;
  float* vs = g.vs;
  float* red = g.red;
  // ---- coin and MH uniform of the workgroup's chains, then the row's direction ----
  if (tid < w.cpw) {
    const int64_t chain = w.cbase + tid;
    const bool lv = chain < p.step_Bl;        // (streams are indexed by the chain's place in the WHOLE batch)
    w.scoin[tid] = lv ? philox_u01(p.step_seed, (uint64_t)(p.step_chain0 + chain), 2 * p.step_draw + 1) : 1.f;
    w.su[tid] = lv ? philox_u01(p.step_seed, (uint64_t)(p.step_B + p.step_chain0 + chain), 2 * p.step_draw + 1) : 1.f;
  }
  __syncthreads();
  const int d = w.paired ? (r >= w.cpw ? 1 : 0) : (w.scoin[k] > 0.5f ? 0 : 1);     // gauge_dynamics.py:221-227

  // ---- the momenta of the thread's links; the step's input is kept for the reject branch and the observables ----
  float v0[SPT], v1[SPT], xi0[SPT], xi1[SPT];
#pragma unroll
  for (int j = 0; j < SPT; ++j) {
    v0[j] = v1[j] = 0.f;
    if (g.ok[j] && live) {
      const int s = fl + j * tpc;
      // momenta of (direction d, chain): elements [(d * B + chain) * D, + D) of the normal stream; D is even, so
      // the two links of a site are one Box-Muller pair of one Philox block
      const uint64_t e = ((uint64_t)d * (uint64_t)p.step_B + (uint64_t)(p.step_chain0 + grow)) * (uint64_t)D + 2 * s;
      const uint64_t nb = e >> 2;
      uint32_t c[4] = {(uint32_t)nb, (uint32_t)(nb >> 32), (uint32_t)(2 * p.step_draw), (uint32_t)((2 * p.step_draw) >> 32)};
      philox4x32_10(c, (uint32_t)p.step_seed, (uint32_t)(p.step_seed >> 32));
      float nv[4];
      philox_normal4(c, nv);
      const bool hi = (e & 2) != 0;
      v0[j] = hi ? nv[2] : nv[0];
      v1[j] = hi ? nv[3] : nv[1];
    }
    xi0[j] = x0[j];
    xi1[j] = x1[j];
  }

  const float pr = hmc_trajectory<SPT, HOLD_LDS>(p, g, be, d, true, x0, x1, v0, v1);

  // ---- mix the directions, Metropolis-Hastings (gauge_dynamics.py:221-257, mask * a + (1 - mask) * b) ----
  // xs rows hold the final x already (published ahead of the last sin P pass); v rows and p join them
  float* vrow = vs + r * D;
#pragma unroll
  for (int j = 0; j < SPT; ++j)
    if (g.ok[j]) {
      vrow[fl + j * tpc] = v0[j];
      vrow[sites + fl + j * tpc] = v1[j];
    }
  if (fl == 0) w.spx[r] = pr;
  __syncthreads();
  const bool primary = r < w.cpw;            // the thread that finishes its links of chain k
  float xo0[SPT], xo1[SPT];
  if (primary) {
    const float fm = w.scoin[k] > 0.5f ? 1.f : 0.f, bm = 1.f - fm;
    const float pk = w.paired ? fm * w.spx[k] + bm * w.spx[k + w.cpw] : w.spx[k];
    const float am = pk > w.su[k] ? 1.f : 0.f;                       // strict >, quirk Q5
    if (fl == 0) w.sobs[k * 4 + 3] = pk;
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      xo0[j] = xo1[j] = 0.f;
      if (g.ok[j]) {
        const int s = fl + j * tpc, c = 2 * s;
        float xp0 = x0[j], xp1 = x1[j], vp0 = v0[j], vp1 = v1[j];
        if (w.paired) {
          const float* xb = xs + (k + w.cpw) * D;
          const float* vb = vs + (k + w.cpw) * D;
          xp0 = fm * xp0 + bm * xb[s];
          xp1 = fm * xp1 + bm * xb[sites + s];
          vp0 = fm * vp0 + bm * vb[s];
          vp1 = fm * vp1 + bm * vb[sites + s];
        }
        xo0[j] = am * xp0 + (1.f - am) * xi0[j];
        xo1[j] = am * xp1 + (1.f - am) * xi1[j];
        if (live) {                                                  // apply_transition's own outputs (:259)
          const int64_t o = grow * D + c;
          if (p.step_xprop) { p.step_xprop[o] = xp0; p.step_xprop[o + 1] = xp1; }
          if (p.step_vprop) { p.step_vprop[o] = vp0; p.step_vprop[o + 1] = vp1; }
          if (p.step_xout) { p.step_xout[o] = xo0[j]; p.step_xout[o + 1] = xo1[j]; }
        }
      }
    }
  }
  __syncthreads();
  // ---- observables of the step's INPUT samples (gauge_model.py:256-266) and the charge of its output (:718-725):
  //      x_in -> the chain's (forward) x row, x_out -> its backward x row, or its v row without one
  float* gin = xs + k * D;
  float* gout = w.paired ? xs + (k + w.cpw) * D : vs + k * D;
  if (primary) {
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      if (g.ok[j]) {
        const int s = fl + j * tpc;
        gin[s] = xi0[j];
        gin[sites + s] = xi1[j];
        gout[s] = xo0[j];
        gout[sites + s] = xo1[j];
      }
    }
  }
  __syncthreads();
  auto plaq = [&](const float* xc, float& scos, float& sproj) {
    const float inv2pi = 0.15915494309189533577f;
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      if (g.ok[j]) {
        const int s = fl + j * tpc;
        const float P = xc[s] - xc[sites + s] - xc[g.nr[j]] + xc[sites + g.nu[j]];
        float sn, cs;
        fast_sincos(P, &sn, &cs);
        a += cs;
        b += P - 6.28318530717958647692f * floorf((P + 3.14159265358979323846f) * inv2pi);   // project_angle
      }
    }
    scos = a;
    sproj = b;
  };
  if (w.paired) {
    float a, b;
    plaq(primary ? gin : gout, a, b);
    hmc_row_sum2(a, b, tsh, r, fl, red);
    if (fl == 0) {
      if (primary) { w.sobs[k * 4 + 0] = a; w.sobs[k * 4 + 1] = b; }
      else w.sobs[k * 4 + 2] = b;
    }
  } else {
    float a, b, c_, d_;
    plaq(gin, a, b);
    plaq(gout, c_, d_);
    hmc_row_sum2(a, b, tsh, r, fl, red);
    hmc_row_sum2(c_, d_, tsh, r, fl, red);
    if (fl == 0) { w.sobs[k * 4 + 0] = a; w.sobs[k * 4 + 1] = b; w.sobs[k * 4 + 2] = d_; }
  }
  __syncthreads();
  if (tid < w.cpw) {
    const float inv2pi = 0.15915494309189533577f;
    const int64_t chain = w.cbase + tid;
    if (chain < p.step_Bl) {
      const float q_in = w.sobs[tid * 4 + 1] * inv2pi, q_out = w.sobs[tid * 4 + 2] * inv2pi;
      if (p.step_px) p.step_px[chain] = w.sobs[tid * 4 + 3];
      if (p.step_act) p.step_act[chain] = (float)sites - w.sobs[tid * 4 + 0];      // sum (1 - cos P)
      if (p.step_plq) p.step_plq[chain] = w.sobs[tid * 4 + 0] / (float)sites;
      if (p.step_chg) p.step_chg[chain] = q_in;
      if (p.step_dq) p.step_dq[chain] = fabsf(q_in - q_out);
    }
  }
  // ---- np.mod(x_out, 2 pi) (gauge_model.py:1388): the chains' new state, to registers and to step_x_next; then
  //      the step's sums ----
  if (primary) {
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      x0[j] = x1[j] = 0.f;
      if (g.ok[j]) {
        float wv[2] = {xo0[j], xo1[j]};
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const float tp = 6.28318530717958647692f;
          float m_ = fmaf(-tp, floorf(wv[e] * 0.15915494309189533577f), wv[e]);       // w - 2 pi floor(w / 2 pi)
          if (m_ < 0.f) m_ += tp;
          if (m_ >= tp) m_ -= tp;
          wv[e] = m_;
        }
        x0[j] = wv[0];
        x1[j] = wv[1];
        if (live && p.step_x_next) {
          float* xn = p.step_x_next + grow * D + 2 * (fl + j * tpc);
          xn[0] = wv[0];
          xn[1] = wv[1];
        }
      }
    }
  }
  step_sums<kHmcMaxThreads, 256>(p, w, ngrp, (int64_t)blockIdx.x * ngrp, npart, (int)gridDim.x, g.fin);
}

template <int SPT>
__global__ __launch_bounds__(kHmcMaxThreads) void hmc_step_kernel(const FusedArgs p, const int tsh) {
  extern __shared__ float lds[];
  const HmcLanes<SPT> g = hmc_lanes<SPT>(p, tsh, lds, (int)threadIdx.x);
  const StepWg w = hmc_workgroup<SPT>(p, g);
  float x0[SPT], x1[SPT];
  if (w.stepm) {
    int k;
    int64_t grow;
    bool live;
    hmc_step_row<SPT>(p, g, w, k, grow, live);
    hmc_load_x<SPT>(p, g, grow, live, x0, x1);
    hmc_step<SPT, true>(p, g, w, HmcRowValues{p.beta, p.eps}, k, grow, live, x0, x1, 1, (int)gridDim.x);
    return;
  }
  // ---- trajectory mode: x, v, sumlogdet (exactly 0), p of the live rows ----
  const int64_t grow = w.row0 + g.r;
  const bool live = g.r < w.nrow;
  const int d = live && p.dir ? p.dir[grow] : 0;
  float v0[SPT], v1[SPT];
  hmc_load_x<SPT>(p, g, grow, live, x0, x1);
#pragma unroll
  for (int j = 0; j < SPT; ++j) {
    v0[j] = v1[j] = 0.f;
    if (g.ok[j] && live) {
      const float* vr = p.v0 + grow * g.D + 2 * (g.fl + j * g.tpc);
      v0[j] = vr[0];
      v1[j] = vr[1];
    }
  }
  const float pr =
      hmc_trajectory<SPT, true>(p, g, HmcRowValues{p.beta, p.eps}, d, p.p_accept != nullptr, x0, x1, v0, v1);
  if (live) {
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      if (g.ok[j]) {
        float* xo = p.x_out + grow * g.D + 2 * (g.fl + j * g.tpc);
        float* vo = p.v_out + grow * g.D + 2 * (g.fl + j * g.tpc);
        xo[0] = x0[j];
        xo[1] = x1[j];
        vo[0] = v0[j];
        vo[1] = v1[j];
      }
    }
    if (g.fl == 0) {
      if (p.logdet && !p.logdet_accumulate) p.logdet[grow] = 0.f;
      if (p.p_accept) p.p_accept[grow] = pr;
    }
  }
}

// What a RUN of MCMC steps adds to FusedArgs (l2hmc_gauge_hmc_run).  FusedArgs holds the run's first draw index
// (step_draw), the first row of every history (step_px ... step_dq, step_sums, step_part) and the final state
// (step_x_next); step s of the run uses draw step_draw + s, betas[s] and the rows s of the histories.
// PRECONDITION, checked on the host by l2hmc_gauge_hmc_run and launch_hmc_run before the launch:
// step_draw + n_steps <= 2^63, i.e. bit 63 of every step's draw index is 0.  hmc_run_kernel adds that bit to the
// thread's lane, row and chain indices as a zero the compiler cannot fold (see its step loop); were it 1, every
// index would be one too far.
struct HmcRunArgs {
  int n_steps;
  const float* betas;                    // [n_steps]
  int64_t hist_stride;                   // floats between two steps' rows of px / actions / plaqs / charges / charge_diff
  int64_t part_stride;                   // floats between two steps' slices of step_part
  float* samples;                        // [n_steps][sample_stride]: every step's wrapped output, or NULL
  int64_t sample_stride;
};

// What the LADDER form of the run adds (l2hmc_gauge_hmc_run_ladder): beta and the step size get a chain axis.  Step s
// of chain c runs at betas[s * step_stride + c * chain_stride] and chain c integrates with eps_chain[c] (NULL: the
// plan's eps for every chain).  Only the ladder instances take this struct, so the uniform instances keep their
// kernel arguments.
struct HmcLadderArgs : HmcRunArgs {
  int64_t step_stride, chain_stride;     // elements of betas between two steps / two chains; either may be 0
  const float* eps_chain;                // [B], or NULL
};

// n_steps MCMC steps in ONE launch: chains never meet, so a workgroup walks its own chains through the whole run with
// their state in registers.  Step s + 1 starts from the wrapped output of step s -- the fp32 values the step kernel
// stores and its next launch reloads -- and forms everything else anew, so the run gives the bits of n_steps launches
// of hmc_step_kernel.  Workgroups drift apart freely: the only thing that crosses them is a step's sums, and every
// step has a ticket (step_sums[s][3]) and a slice of step_part of its own, so nobody waits for anybody.
// LADDER: beta and eps belong to the CHAIN (HmcLadderArgs).  Both rows of a chain of the paired layout read the same
// pair, so both half-kicks, both position sub-updates and both ends of the Hamiltonian difference of a chain see one
// beta and one eps; a row whose chain is beyond step_Bl reads neither array.  The step is the same copy run on per-row
// values instead of uniform ones: the same fp32 operations in the same order, so a column of a ladder has the bits of
// the uniform run at its (beta, eps).
template <int SPT, bool LADDER>
__global__ __launch_bounds__(kHmcMaxThreads) void hmc_run_kernel(
    const FusedArgs p, const typename std::conditional<LADDER, HmcLadderArgs, HmcRunArgs>::type ra, const int tsh) {
  extern __shared__ float lds[];
  constexpr int kExtra = LADDER ? hmc_ladder_lds_floats(SPT) : 0;
  const HmcLanes<SPT> g = hmc_lanes<SPT>(p, tsh, lds, (int)threadIdx.x, kExtra);
  const StepWg w = hmc_workgroup<SPT>(p, g);
  int k;
  int64_t grow;
  bool live;
  hmc_step_row<SPT>(p, g, w, k, grow, live);
  float x0[SPT], x1[SPT];
  hmc_load_x<SPT>(p, g, grow, live, x0, x1);
  const bool primary = g.r < w.cpw;
  FusedArgs q = p;
  q.step_xprop = q.step_vprop = q.step_xout = nullptr;       // a run has no use for apply_transition's own outputs
  q.step_sums_acc = 0;
  for (int s = 0; s < ra.n_steps; ++s) {
    if constexpr (!LADDER) q.beta = ra.betas[s];
    q.step_draw = p.step_draw + (unsigned long long)s;
    q.step_x_next = ra.samples ? ra.samples + s * ra.sample_stride : nullptr;
    q.step_px = p.step_px ? p.step_px + s * ra.hist_stride : nullptr;
    q.step_act = p.step_act ? p.step_act + s * ra.hist_stride : nullptr;
    q.step_plq = p.step_plq ? p.step_plq + s * ra.hist_stride : nullptr;
    q.step_chg = p.step_chg ? p.step_chg + s * ra.hist_stride : nullptr;
    q.step_dq = p.step_dq ? p.step_dq + s * ra.hist_stride : nullptr;
    q.step_sums = p.step_sums ? p.step_sums + 4 * (int64_t)s : nullptr;
    q.step_part = p.step_part ? p.step_part + s * ra.part_stride : nullptr;
    // The step's LDS and global addresses are all formed from the thread's lane and row.  Left to itself the compiler
    // forms every one of them ahead of the loop and keeps them in registers across it: twice the step kernel's
    // VGPRs, half its workgroups per CU.  z is 0 (a draw index does not reach 2^63), which the compiler cannot know,
    // so the addresses are formed where they are used, as in the step kernel; the neighbour tables stay hoisted.
    // The host refuses a run whose draw indices reach 2^63 (HmcRunArgs).  The register counts depend on the compiler:
    // 75 / 93 / 127 VGPRs (SPT 1 / 2 / 4), no scratch, with hipcc of ROCm 7.2.0 (HIP 7.2.26015, AMD clang 22.0.0git roc-7.2.0) at -O3;
    // the ladder instances 77 / 95 / 126 (profiles/hmc_run_ladder.txt, taken three registers earlier at SPT 1 and 2).
    const int z = (int)(q.step_draw >> 63);
    HmcLanes<SPT> gs = g;
    if (SPT == 4) {
      // four sites per thread: the 20 registers of the neighbour tables would cost the second workgroup of a CU
      // (136 VGPRs with them hoisted, 127 without), so this instance forms them per step as well
      gs = hmc_lanes<SPT>(p, tsh, lds, (int)threadIdx.x + z, kExtra);
    } else {
      gs.fl = g.fl + z;
      gs.r = g.r + z;
      gs.xrow = g.xs + gs.r * g.D;
      gs.sprow = g.sp + gs.r * g.sites;
    }
    StepWg ws = w;
    ws.tid = w.tid + z;
    if constexpr (LADDER) {
      // the pair of the row's chain, read where the step starts (two cached loads per row and step) so that neither is
      // live across the step's epilogue; the chain's index is formed here like every other address of the step.  A dead
      // row (x = v = 0) reads neither array.
      const int64_t c = grow + z;
      const float beta = live ? ra.betas[s * ra.step_stride + c * ra.chain_stride] : 0.f;
      const float eps = live && ra.eps_chain ? ra.eps_chain[c] : p.eps;
      if constexpr (kExtra != 0) {
        // 127 VGPRs without the pair, 128 is what two workgroups per CU allow (130 with the pair in registers): the
        // pair waits in the row's LDS scratch, 126 VGPRs.
        // The step's first barrier (after the coins) comes ahead of the trajectory's first read, and the barriers of
        // the step's epilogue come between the trajectory's last read and the next step's write.
        float* rb = gs.stp + 8 * gs.R + 2 * gs.r;
        if (gs.fl == 0) {
          rb[0] = beta;
          rb[1] = eps;
        }
        hmc_step<SPT, SPT != 4>(q, gs, ws, HmcRowLds{rb}, k + z, c, live, x0, x1, 1, (int)gridDim.x);
      } else {
        hmc_step<SPT, SPT != 4>(q, gs, ws, HmcRowValues{beta, eps}, k + z, c, live, x0, x1, 1, (int)gridDim.x);
      }
    } else {
      hmc_step<SPT, SPT != 4>(q, gs, ws, HmcRowValues{q.beta, q.eps}, k + z, grow + z, live, x0, x1, 1, (int)gridDim.x);
    }
    if (w.paired) {
      // the chain's new state is in its forward row's registers: hand it to the backward row through that row's
      // own (free) x row.  The next write there is the backward row's own publish of the same values.
      if (primary) {
        float* xb = gs.xs + (k + z + w.cpw) * gs.D;
#pragma unroll
        for (int j = 0; j < SPT; ++j)
          if (gs.ok[j]) {
            xb[gs.fl + j * gs.tpc] = x0[j];
            xb[gs.sites + gs.fl + j * gs.tpc] = x1[j];
          }
      }
      __syncthreads();
      if (!primary) {
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
          x0[j] = x1[j] = 0.f;
          if (gs.ok[j]) {
            x0[j] = gs.xrow[gs.fl + j * gs.tpc];
            x1[j] = gs.xrow[gs.sites + gs.fl + j * gs.tpc];
          }
        }
      }
    }
  }
  if (primary && live && p.step_x_next) {
#pragma unroll
    for (int j = 0; j < SPT; ++j)
      if (g.ok[j]) {
        float* xn = p.step_x_next + grow * g.D + 2 * (g.fl + j * g.tpc);
        xn[0] = x0[j];
        xn[1] = x1[j];
      }
  }
}

static int launch_hmc(const FusedArgs& a, const HmcGeom& g, int64_t nwg, hipStream_t stream,
                      const HmcRunArgs* run = nullptr, const HmcLadderArgs* ladder = nullptr) {
  L2HMC_REQUIRE(nwg > 0 && nwg < (1ll << 31), "hmc step: too many rows");
  prof_before(kProfFused, stream);
  const dim3 grid((unsigned)nwg), block((unsigned)g.threads);
  if (ladder) {
    const size_t lds = g.lds + sizeof(float) * (size_t)(g.rows_wg * hmc_ladder_lds_floats(g.spt));
    if (g.spt == 1)
      hipLaunchKernelGGL((hmc_run_kernel<1, true>), grid, block, lds, stream, a, *ladder, g.tsh);
    else if (g.spt == 2)
      hipLaunchKernelGGL((hmc_run_kernel<2, true>), grid, block, lds, stream, a, *ladder, g.tsh);
    else
      hipLaunchKernelGGL((hmc_run_kernel<4, true>), grid, block, lds, stream, a, *ladder, g.tsh);
  } else if (run) {
    if (g.spt == 1)
      hipLaunchKernelGGL((hmc_run_kernel<1, false>), grid, block, g.lds, stream, a, *run, g.tsh);
    else if (g.spt == 2)
      hipLaunchKernelGGL((hmc_run_kernel<2, false>), grid, block, g.lds, stream, a, *run, g.tsh);
    else
      hipLaunchKernelGGL((hmc_run_kernel<4, false>), grid, block, g.lds, stream, a, *run, g.tsh);
  } else if (g.spt == 1)
    hipLaunchKernelGGL((hmc_step_kernel<1>), grid, block, g.lds, stream, a, g.tsh);
  else if (g.spt == 2)
    hipLaunchKernelGGL((hmc_step_kernel<2>), grid, block, g.lds, stream, a, g.tsh);
  else
    hipLaunchKernelGGL((hmc_step_kernel<4>), grid, block, g.lds, stream, a, g.tsh);
  prof_after(kProfFused, stream);
  L2HMC_CHECK_LAUNCH("hmc_step");
  return L2HMC_OK;
}

int launch_hmc_trajectory(const l2hmc_gauge_plan* p, float beta, int step_begin, int step_end, const float* x0,
                          const float* v0, const int* dir, int64_t rows, float* x_out, float* v_out, float* logdet,
                          int logdet_accumulate, float* p_accept, hipStream_t stream) {
  HmcGeom g;
  L2HMC_REQUIRE(hmc_plan_supported(p) && hmc_geom(p->T, p->X, &g), "hmc trajectory: plan has no one-launch kernel");
  L2HMC_REQUIRE(x0 && v0 && x_out && v_out && rows > 0, "hmc trajectory: bad arguments");
  FusedArgs a{};
  a.T = p->T; a.X = p->X; a.num_steps = p->num_steps; a.step_begin = step_begin; a.step_end = step_end;
  a.eps = p->eps; a.beta = beta; a.masks = p->masks;
  a.x0 = x0; a.v0 = v0; a.dir = dir; a.rows = rows; a.x_out = x_out; a.v_out = v_out;
  a.logdet = logdet; a.logdet_accumulate = logdet_accumulate; a.p_accept = p_accept;
  return launch_hmc(a, g, ceil_div(rows, g.rows_wg), stream);
}

int launch_hmc_step(const l2hmc_gauge_plan* p, float beta, const float* x_in, float* x_next, int64_t B, uint64_t seed,
                    uint64_t draw, int both, float* px, float* actions, float* plaqs, float* charges, float* dq,
                    float* step_sums, float* part, hipStream_t stream, float* x_prop, float* v_prop, float* x_out) {
  HmcGeom g;
  L2HMC_REQUIRE(hmc_plan_supported(p) && hmc_geom(p->T, p->X, &g), "hmc step: plan has no one-launch kernel");
  L2HMC_REQUIRE(x_in && (x_next || x_out) && B > 0 && (!step_sums || part), "hmc step: bad arguments");
  const int cpw = both ? g.rows_wg / 2 : g.rows_wg;
  const int64_t nwg = ceil_div(B, cpw);
  FusedArgs a{};
  a.T = p->T; a.X = p->X; a.num_steps = p->num_steps; a.step_begin = 0; a.step_end = p->num_steps;
  a.eps = p->eps; a.beta = beta; a.masks = p->masks;
  a.x0 = x_in; a.rows = nwg * g.rows_wg;
  a.step_x_next = x_next; a.step_xprop = x_prop; a.step_vprop = v_prop; a.step_xout = x_out;
  a.step_B = B; a.step_Bl = B; a.step_chain0 = 0;
  a.step_seed = seed; a.step_draw = draw; a.step_both = both;
  a.step_px = px; a.step_act = actions; a.step_plq = plaqs; a.step_chg = charges; a.step_dq = dq;
  a.step_sums = step_sums; a.step_part = part;       // part: 2 floats per workgroup
  return launch_hmc(a, g, nwg, stream);
}

size_t hmc_run_part_bytes(int64_t B) { return align_up(sizeof(float) * 2 * (size_t)B, 256); }

// the FusedArgs and HmcRunArgs of a run, uniform or ladder (the ladder form's own three fields are its launcher's)
static int hmc_run_args(const l2hmc_gauge_plan* p, const float* betas, const float* x_in, float* x_next, int64_t B,
                        uint64_t seed, uint64_t draw0, int n_steps, int both, float* px, float* actions, float* plaqs,
                        float* charges, float* dq, float* step_sums, float* samples, float* part, HmcGeom* g,
                        int64_t* nwg, FusedArgs* a, HmcRunArgs* r) {
  L2HMC_REQUIRE(hmc_plan_supported(p) && hmc_geom(p->T, p->X, g), "hmc run: plan has no one-launch kernel");
  L2HMC_REQUIRE(betas && x_in && x_next && B > 0 && n_steps > 0 && (!step_sums || part), "hmc run: bad arguments");
  L2HMC_REQUIRE(draw0 <= (1ull << 63) - (uint64_t)n_steps, "hmc run: draw0 + n_steps exceeds 2^63");   // HmcRunArgs
  const int cpw = both ? g->rows_wg / 2 : g->rows_wg;
  *nwg = ceil_div(B, cpw);
  const int64_t D = 2 * (int64_t)p->T * p->X;
  a->T = p->T; a->X = p->X; a->num_steps = p->num_steps; a->step_begin = 0; a->step_end = p->num_steps;
  a->eps = p->eps; a->masks = p->masks;
  a->x0 = x_in; a->rows = *nwg * g->rows_wg;
  a->step_x_next = x_next;
  a->step_B = B; a->step_Bl = B; a->step_chain0 = 0;
  a->step_seed = seed; a->step_draw = draw0; a->step_both = both;
  a->step_px = px; a->step_act = actions; a->step_plq = plaqs; a->step_chg = charges; a->step_dq = dq;
  a->step_sums = step_sums; a->step_part = part;     // part: hmc_run_part_bytes(B) per step (2 floats per workgroup)
  r->n_steps = n_steps; r->betas = betas; r->hist_stride = B;
  r->part_stride = (int64_t)(hmc_run_part_bytes(B) / sizeof(float));
  r->samples = samples; r->sample_stride = B * D;
  return L2HMC_OK;
}

int launch_hmc_run(const l2hmc_gauge_plan* p, const float* betas, const float* x_in, float* x_next, int64_t B,
                   uint64_t seed, uint64_t draw0, int n_steps, int both, float* px, float* actions, float* plaqs,
                   float* charges, float* dq, float* step_sums, float* samples, float* part, hipStream_t stream) {
  HmcGeom g;
  int64_t nwg;
  FusedArgs a{};
  HmcRunArgs r{};
  if (int e = hmc_run_args(p, betas, x_in, x_next, B, seed, draw0, n_steps, both, px, actions, plaqs, charges, dq,
                           step_sums, samples, part, &g, &nwg, &a, &r))
    return e;
  return launch_hmc(a, g, nwg, stream, &r);
}

int launch_hmc_run_ladder(const l2hmc_gauge_plan* p, const float* betas, int64_t step_stride, int64_t chain_stride,
                          const float* eps_chain, const float* x_in, float* x_next, int64_t B, uint64_t seed,
                          uint64_t draw0, int n_steps, int both, float* px, float* actions, float* plaqs,
                          float* charges, float* dq, float* step_sums, float* samples, float* part,
                          hipStream_t stream) {
  HmcGeom g;
  int64_t nwg;
  FusedArgs a{};
  HmcLadderArgs r{};
  L2HMC_REQUIRE(step_stride >= 0 && chain_stride >= 0, "hmc run: negative stride");
  if (int e = hmc_run_args(p, betas, x_in, x_next, B, seed, draw0, n_steps, both, px, actions, plaqs, charges, dq,
                           step_sums, samples, part, &g, &nwg, &a, &r))
    return e;
  r.step_stride = step_stride; r.chain_stride = chain_stride; r.eps_chain = eps_chain;
  return launch_hmc(a, g, nwg, stream, nullptr, &r);
}

// ---- the ladder run with the replica-exchange rounds INSIDE the launch (l2hmc_gauge_hmc_run_exchange) ----
// A round is the one stage in which chains meet.  hmc_run_kernel's workgroups are sized by the lattice, so a pair of
// rungs may sit in two of them and a round between its steps would need a grid-wide wait.  This instance sizes the
// workgroup by the REPLICA GROUP instead: cpw = lcm(group, cpw0) chains (cpw0: the chains of a ladder-run workgroup),
// i.e. a whole number of groups and a whole number of the ladder run's workgroups, with the same row layout (forward
// rows [0, cpw), backward rows [cpw, 2 cpw)).  Every pair then sits in ONE workgroup and meets at __syncthreads():
// nothing crosses workgroups, nobody spins, no co-residency is assumed.  A (lattice, group) whose workgroup would exceed
// 1024 threads is not served (hmc_exchange_geom); l2hmc_gauge_replica_swap between launches takes it.
//   * The step is hmc_step, the one copy; the workgroup leaves the partial sums of the ngrp = cpw / cpw0 ladder-run
//     workgroups it stands for, so step_sums come out bit for bit.
//   * The round (after step s iff (swap_phase + s + 1) % swap_every == 0) acts on the wrapped state in the primary
//     rows' registers at the betas step s ran with: the rows publish x to their LDS planes, form S in the order of
//     replica_swap_kernel (gauge_swap.h), decide with gauge_swap.h's rule, and on accept the two chains' threads take
//     each other's x from the planes.  Labels travel in a register per chain thread and through LDS.
//   * Every barrier of the round is reached by every thread of the workgroup: backward rows, dead rows, lanes beyond
//     the lattice and chains that sit a round out go through them; the round's only conditions around a barrier are
//     uniform over the grid (the round's schedule, tsh).
//   * Streams: a step at draw index d takes 2 d and 2 d + 1, a round after it 2 d + 2, and the next step is d + 2
//     (2 d + 3 is skipped) -- the loop `run_hmc(k)`, `swap_replicas` on one counter.  A pairless round (group 2 at parity
//     1) takes its stream too.  PRECONDITION (host): step_draw + n_steps + rounds <= 2^63, HmcRunArgs' bit-63 rule.
//   * Registers (hipcc of ROCm 7.2.0 at -O3, profiles/hmc_run_exchange.txt): 97 / 117 VGPRs at SPT 1 / 2, no scratch,
//     under the 128 that sixteen waves per CU leave.  SPT 4 (513 .. 1024 sites) takes 128 VGPRs AND scratch -- its
//     ladder form already sits at 126 --, so it is not shipped: those lattices are not served.  To read its resources,
//     compile this file with -DL2HMC_HMC_EXCHANGE_SPT4 (an explicit instantiation at the end of the file, nothing else).
constexpr int kHmcExchangeThreads = 1024;
constexpr int kHmcExchangeSpt = 2;        // the largest SPT with an instance that is launched

struct HmcExchangeArgs : HmcLadderArgs {
  int group, swap_every, swap_phase, first_parity;
  int ngrp, npart;                       // step_sums: slots per workgroup, and the ladder run's grid size
  int32_t* replica;                      // [B] labels, read on entry and written on exit, or NULL (labels start as the column)
  float* swap_p;                         // [rounds][B] or NULL
  uint8_t* swapped;                      // [rounds][B] or NULL
  int32_t* replica_hist;                 // [rounds][B] or NULL
};

template <int SPT>
__global__ __launch_bounds__(kHmcExchangeThreads) void hmc_run_exchange_kernel(const FusedArgs p,
                                                                               const HmcExchangeArgs ra,
                                                                               const int tsh) {
  extern __shared__ float lds[];
  const HmcLanes<SPT> g = hmc_lanes<SPT>(p, tsh, lds, (int)threadIdx.x);
  const StepWg w = hmc_workgroup<SPT>(p, g);
  int k;
  int64_t grow;
  bool live;
  hmc_step_row<SPT>(p, g, w, k, grow, live);
  float x0[SPT], x1[SPT];
  hmc_load_x<SPT>(p, g, grow, live, x0, x1);
  const bool primary = g.r < w.cpw;
  float* sS = g.fin + 2 * 256;                                       // [R] S of the workgroup's chains
  int32_t* sLab = reinterpret_cast<int32_t*>(sS + g.R);              // [R] their labels
  int32_t label = primary && live ? (ra.replica ? ra.replica[grow] : (int32_t)grow) : 0;
  FusedArgs q = p;
  q.step_xprop = q.step_vprop = q.step_xout = nullptr;
  q.step_sums_acc = 0;
  unsigned long long draw = p.step_draw;
  int jr = 0;                                                        // rounds of this launch so far
  for (int s = 0; s < ra.n_steps; ++s) {
    q.step_draw = draw;
    q.step_x_next = ra.samples ? ra.samples + s * ra.sample_stride : nullptr;
    q.step_px = p.step_px ? p.step_px + s * ra.hist_stride : nullptr;
    q.step_act = p.step_act ? p.step_act + s * ra.hist_stride : nullptr;
    q.step_plq = p.step_plq ? p.step_plq + s * ra.hist_stride : nullptr;
    q.step_chg = p.step_chg ? p.step_chg + s * ra.hist_stride : nullptr;
    q.step_dq = p.step_dq ? p.step_dq + s * ra.hist_stride : nullptr;
    q.step_sums = p.step_sums ? p.step_sums + 4 * (int64_t)s : nullptr;
    q.step_part = p.step_part ? p.step_part + s * ra.part_stride : nullptr;
    // z is 0: the addresses of the step are formed where they are used (hmc_run_kernel's step loop)
    const int z = (int)(q.step_draw >> 63);
    HmcLanes<SPT> gs = g;
    gs.fl = g.fl + z;
    gs.r = g.r + z;
    gs.xrow = g.xs + gs.r * g.D;
    gs.sprow = g.sp + gs.r * g.sites;
    StepWg ws = w;
    ws.tid = w.tid + z;
    const int kz = k + z;
    const int64_t c = grow + z;
    const float* bs = ra.betas + s * ra.step_stride;
    {
      // the pair of the row's chain, as the ladder run reads it; a dead row (x = v = 0) reads neither array
      const float beta = live ? bs[c * ra.chain_stride] : 0.f;
      const float eps = live && ra.eps_chain ? ra.eps_chain[c] : p.eps;
      hmc_step<SPT, SPT != 4>(q, gs, ws, HmcRowValues{beta, eps}, kz, c, live, x0, x1, ra.ngrp, ra.npart);
    }
    const bool round = (ra.swap_phase + s + 1) % ra.swap_every == 0;  // uniform over the grid
    if (round) {
      const int parity = (ra.first_parity + jr) & 1;
      // the primary rows' planes are free: the step's last reads of them lie behind its last barrier
      if (primary) {
#pragma unroll
        for (int j = 0; j < SPT; ++j)
          if (gs.ok[j]) {
            gs.xrow[gs.fl + j * gs.tpc] = x0[j];
            gs.xrow[gs.sites + gs.fl + j * gs.tpc] = x1[j];
          }
        if (gs.fl == 0) sLab[kz] = label;
      }
      __syncthreads();
      // S of the row: the thread's plaquettes in ascending order, wave_sum, the waves in ascending order
      float a = 0.f;
      if (primary) {
#pragma unroll
        for (int j = 0; j < SPT; ++j)
          if (gs.ok[j]) a += gauge_swap_term(x0[j], x1[j], gs.xrow[gs.nr[j]], gs.xrow[gs.sites + gs.nu[j]]);
      }
      if (tsh < 6) {
        a = gauge_swap_subwave_sum(a, tsh);
      } else {
        a = wave_sum(a);
        if (tsh > 6) {
          if ((gs.fl & (kWave - 1)) == 0) gs.red[(gs.r * 4 + (gs.fl >> 6)) * 2] = a;
          __syncthreads();
          a = gauge_swap_add_waves(gs.red + gs.r * 8, 2, 0, 1 << (tsh - 6));
        }
      }
      if (primary && gs.fl == 0) sS[kz] = a;
      __syncthreads();
      // cbase is a multiple of cpw and cpw of the group: the slot gives the rung, and a pair has both chains here and,
      // as B is a multiple of the group, both live or both dead
      const int jg = kz % ra.group;
      const bool lower = gauge_swap_lower(jg, ra.group, parity), upper = gauge_swap_upper(jg, parity);
      if (primary && live) {
        bool acc = false;
        float pp = 0.f;
        if (lower || upper) {
          const int ka = upper ? kz - 1 : kz;                         // the pair's lower chain
          const int64_t ca = w.cbase + ka;
          acc = gauge_swap_decide(bs[ca * ra.chain_stride], bs[(ca + 1) * ra.chain_stride], sS[ka], sS[ka + 1],
                                  p.step_seed, (uint64_t)(p.step_chain0 + ca), 2 * draw + 2, &pp);
        }
        if (acc) {
          const int ko = upper ? kz - 1 : kz + 1;
          const float* xo = gs.xs + ko * gs.D;
#pragma unroll
          for (int j = 0; j < SPT; ++j)
            if (gs.ok[j]) {
              x0[j] = xo[gs.fl + j * gs.tpc];
              x1[j] = xo[gs.sites + gs.fl + j * gs.tpc];
            }
          label = sLab[ko];
        }
        if (gs.fl == 0) {
          const int64_t row = (int64_t)jr * p.step_B;
          gauge_swap_outputs(ra.swap_p ? ra.swap_p + row : nullptr, ra.swapped ? ra.swapped + row : nullptr, c, lower,
                             pp, acc);
          if (ra.replica_hist) ra.replica_hist[row + c] = label;
        }
      }
      ++jr;
      // the next write to a primary row's planes, sS or sLab lies behind the barrier below (paired layout) or behind
      // the next step's first barrier
    }
    draw += round ? 2ull : 1ull;
    if (w.paired) {
      if (primary) {
        float* xb = gs.xs + (kz + w.cpw) * gs.D;
#pragma unroll
        for (int j = 0; j < SPT; ++j)
          if (gs.ok[j]) {
            xb[gs.fl + j * gs.tpc] = x0[j];
            xb[gs.sites + gs.fl + j * gs.tpc] = x1[j];
          }
      }
      __syncthreads();
      if (!primary) {
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
          x0[j] = x1[j] = 0.f;
          if (gs.ok[j]) {
            x0[j] = gs.xrow[gs.fl + j * gs.tpc];
            x1[j] = gs.xrow[gs.sites + gs.fl + j * gs.tpc];
          }
        }
      }
    }
  }
  if (primary && live) {
    if (p.step_x_next) {
#pragma unroll
      for (int j = 0; j < SPT; ++j)
        if (g.ok[j]) {
          float* xn = p.step_x_next + grow * g.D + 2 * (g.fl + j * g.tpc);
          xn[0] = x0[j];
          xn[1] = x1[j];
        }
    }
    if (ra.replica && g.fl == 0) ra.replica[grow] = label;
  }
}

struct HmcExchangeGeom {
  HmcGeom g;
  int cpw0, cpw, threads;                // chains of a ladder-run workgroup, of this one, and its size
  size_t lds;
};

// what a launch gets of dynamic LDS without an opt-in: a shape that needs more is not served (none does but a one-site
// lattice with 768 rows or more per workgroup), so the launch needs no function attribute
constexpr size_t kHmcExchangeLds = 64 * 1024;

// The workgroup of the exchange run for (lattice, both, group), or false with `why` worded: the served rule.
static bool hmc_exchange_geom(int T, int X, int both, int group, HmcExchangeGeom* e, char* why, size_t nwhy) {
  if (T <= 0 || X <= 0) {
    snprintf(why, nwhy, "bad lattice T=%d X=%d", T, X);
    return false;
  }
  if (!hmc_geom(T, X, &e->g)) {
    snprintf(why, nwhy, "the %dx%d lattice has no one-launch kernel (more than %d sites)", T, X, kHmcMaxSites);
    return false;
  }
  const int rpc = both ? 2 : 1, tpc = 1 << e->g.tsh;
  e->cpw0 = e->g.rows_wg / rpc;
  int64_t a = group, b = e->cpw0;
  while (b) {
    const int64_t t = a % b;
    a = b;
    b = t;
  }
  const int64_t cpw = (int64_t)group / a * e->cpw0;                  // lcm(group, cpw0)
  if (cpw * rpc * tpc > kHmcExchangeThreads) {
    snprintf(why, nwhy, "a %dx%d lattice takes %d threads per row and %d row(s) per chain, and a workgroup that holds "
             "whole groups of %d rungs and whole ladder-run workgroups of %d chains has lcm = %lld chains: %lld threads, "
             "more than %d", T, X, tpc, rpc, group, e->cpw0, (long long)cpw, (long long)(cpw * rpc * tpc),
             kHmcExchangeThreads);
    return false;
  }
  if (e->g.spt > kHmcExchangeSpt) {
    snprintf(why, nwhy, "the %dx%d lattice takes %d sites per thread, and that instance of the exchange run does not "
             "fit 128 registers without scratch", T, X, e->g.spt);
    return false;
  }
  e->cpw = (int)cpw;
  e->threads = e->cpw * rpc * tpc;
  const int R = e->cpw * rpc;
  // hmc_geom's carve-up for R rows, and sS, sLab [R] behind the sum tree
  e->lds = sizeof(float) * ((size_t)R * (5 * (size_t)T * X + 8 + 8 + 2) + 2 * 256);
  if (e->lds > kHmcExchangeLds) {
    snprintf(why, nwhy, "the %d rows of a %dx%d lattice that such a workgroup holds take %zu B of LDS, more than the %zu "
             "a launch gets", R, T, X, e->lds, kHmcExchangeLds);
    return false;
  }
  return true;
}

int hmc_exchange_served(const l2hmc_gauge_plan* p, int group, char* why, size_t nwhy) {
  HmcExchangeGeom e;
  if (!p->hmc || p->num_steps <= 0) {
    snprintf(why, nwhy, "plan.hmc = 0 (a run is steps of plain HMC)");
    return 0;
  }
  if (p->flags & L2HMC_PLAN_LAYERED) {
    snprintf(why, nwhy, "the plan is L2HMC_PLAN_LAYERED: it has no one-launch kernel");
    return 0;
  }
  if (group < 2) {
    snprintf(why, nwhy, "group = %d: a replica group has 2 rungs or more", group);
    return 0;
  }
  return hmc_exchange_geom(p->T, p->X, (p->flags & L2HMC_PLAN_SELECTED_ONLY) ? 0 : 1, group, &e, why, nwhy) ? 1 : 0;
}

int launch_hmc_run_exchange(const l2hmc_gauge_plan* p, const float* betas, int64_t step_stride, int64_t chain_stride,
                            const float* eps_chain, const float* x_in, float* x_next, int64_t B, uint64_t seed,
                            uint64_t draw0, int n_steps, int both, int group, int swap_every, int swap_phase,
                            int first_parity, int32_t* replica, float* px, float* actions, float* plaqs,
                            float* charges, float* dq, float* step_sums, float* samples, float* swap_p,
                            uint8_t* swapped, int32_t* replica_hist, float* part, hipStream_t stream) {
  HmcGeom g;
  int64_t nwg0;
  FusedArgs a{};
  HmcExchangeArgs r{};
  HmcExchangeGeom e;
  char why[384];
  L2HMC_REQUIRE(step_stride >= 0 && chain_stride >= 0, "hmc run exchange: negative stride");
  L2HMC_REQUIRE(hmc_exchange_geom(p->T, p->X, both, group, &e, why, sizeof(why)), "hmc run exchange: not served: %s",
                why);
  if (int err = hmc_run_args(p, betas, x_in, x_next, B, seed, draw0, n_steps, both, px, actions, plaqs, charges, dq,
                             step_sums, samples, part, &g, &nwg0, &a, &r))
    return err;
  const int64_t nwg = ceil_div(B, e.cpw);
  L2HMC_REQUIRE(nwg0 < (1ll << 31) && nwg > 0, "hmc run exchange: too many rows");
  a.rows = nwg * (int64_t)(e.threads >> e.g.tsh);
  r.step_stride = step_stride; r.chain_stride = chain_stride; r.eps_chain = eps_chain;
  r.group = group; r.swap_every = swap_every; r.swap_phase = swap_phase; r.first_parity = first_parity;
  r.ngrp = e.cpw / e.cpw0; r.npart = (int)nwg0;
  r.replica = replica; r.swap_p = swap_p; r.swapped = swapped; r.replica_hist = replica_hist;
  prof_before(kProfFused, stream);
  const dim3 grid((unsigned)nwg), block((unsigned)e.threads);
  if (e.g.spt == 1)
    hipLaunchKernelGGL((hmc_run_exchange_kernel<1>), grid, block, e.lds, stream, a, r, e.g.tsh);
  else
    hipLaunchKernelGGL((hmc_run_exchange_kernel<2>), grid, block, e.lds, stream, a, r, e.g.tsh);
  prof_after(kProfFused, stream);
  L2HMC_CHECK_LAUNCH("hmc_run_exchange");
  return L2HMC_OK;
}

#ifdef L2HMC_HMC_EXCHANGE_SPT4
// diagnostic only: the instance that is not shipped, compiled so that the compiler reports its registers and scratch
template __global__ void hmc_run_exchange_kernel<4>(const FusedArgs, const HmcExchangeArgs, const int);
#endif

}  // namespace l2hmc
