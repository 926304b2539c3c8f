// The chain-local stages of the toy-target kernels, the toy family's counterpart of fused_step.h: the staged target,
// the augmented-leapfrog trajectory of one chain (utils/dynamics.py:120-225, :255-319) and the pieces of the sampler
// step around it (utils/sampler.py:28-59).  How a chain is spread over lanes, how a network is evaluated and what is
// staged where stay with the kernels: they hand the trajectory callables.
//
// Who calls this today: small_hmc_run_kernel (small_hmc.hip) and small_ais_run_kernel (small_ais.hip, whose target
// callable interpolates between two SmallTargets), and through small_swap.h's replica-exchange round
// (SmallTarget at temperature 1) small_swap_kernel beside it and the EXCHANGE instances of small_traj_mfma_kernel.  small_traj_mfma_kernel (small_mlp.hip) and the
// forward half of small_train_kernel (small_train.hip) spell the same statements out themselves, in the same order:
//   - taken through small_trajectory, four of the former's 96 instances and nine of the latter's 16 gained scratch or
//     crossed a waves-per-SIMD step;
//   - with its own loop but SmallTarget, mix_dir / mh_accept and one helper each for the first-layer input entry, the
//     heads' lane gather and the S / T / Q finishing, small_traj_mfma_kernel kept its registers, but nine rows of the
//     run tools that run it (propose, run and tempered-run instances) measured 0.7 to 7 % slower than the parent's
//     over three alternating rounds; which of the three ingredients costs it was not found, so its device code is the
//     parent's text (profiles/small_step_one_copy.txt has every figure).
// A change to the loop therefore goes into all three; tests/test_gpu_small_hmc_run.py holds the run kernel to the bits
// of the loop over the trajectory kernel.
#pragma once
#include "small_mlp.h"
#include "lf_update.h"
#include <type_traits>

namespace l2hmc {

// The target as a kernel holds it after its prologue barrier: analytic kind (AN; scalars only), parameters in
// registers (TargetRegs: x_dim <= 2, at most two components) or energy_grad from the LDS image.  The three give the
// same arithmetic in the same order; which one runs is uniform over the launch.
template <int MD, bool AN>
struct SmallTarget {
  static constexpr bool kRegs = !AN && TargetRegs<MD>::kFits;      // (else: no register image to carry)
  struct NoRegs {};
  bool treg = false;
  std::conditional_t<kRegs, TargetRegs<MD>, NoRegs> regs;
  __device__ __forceinline__ void load(const float* Lt, int dim, int K) {
    if constexpr (kRegs) {
      treg = K <= TargetRegs<MD>::KM;
      if (treg) regs.load(Lt, dim, K);
    }
  }
  // E == nullptr: gradient only (inside a trajectory; the energy is needed at its two ends).  Lt, dim, K, tk: the
  // kernel's own values (held here they pin the whole object to memory in the large instances: scratch, registers)
  __device__ __forceinline__ void eval(const float* Lt, int dim, int K, const TargetKind& tk, float inv_temp,
                                       const float (&x)[MD], float* E, float (&g)[MD]) const {
    // rough well / funnel: no parameter arrays, the scalars are kernel arguments -- register-resident at any MD
    if constexpr (AN) {
      analytic_energy_grad<MD>(tk, dim, inv_temp, x, E, g);
      return;
    }
    if constexpr (kRegs) {
      if (treg) {
        regs.eval(dim, K, tk.kind, inv_temp, x, E, g);
        return;
      }
    }
    float dummy;
    energy_grad<MD>(Lt, dim, K, tk, inv_temp, x, E ? E : &dummy, g);
  }
};

// what a trajectory leaves besides (x, v) and the gradient at its end
struct SmallTraj {
  float H0, H1, logdet;        // H = E + |v|^2 / 2 at the two ends, sum of the sub-updates' log-det terms
  // utils/dynamics.py:312-319, one direction
  __device__ __forceinline__ float p_accept() const { return accept_from_delta(H0 - H1 + logdet); }
};

// The networks of plain HMC (utils/dynamics.py:75-78): S = T = Q stay 0 and the compiler folds them.  A type of its
// own, because small_trajectory must not even form the position network's input for it: left to dead-code removal,
// those statements cost small_hmc_run_kernel<2, false, false> three registers (87 -> 90) and 2 % of config 1's time.
template <int MD>
struct NoNet {
  __device__ __forceinline__ void operator()(float, float, const float (&)[MD], const float (&)[MD], float (&)[MD],
                                             float (&)[MD], float (&)[MD]) const {}
};

// One chain from (x, v) through N leapfrog steps in direction bwd; Lm = masks [N][dim].  The caller supplies
//   time(step, tc, ts)                   (cos, sin) of 2 pi step / N
//   netx / netv(tc, ts, a, b, S, T, Q)   the position / momentum network on inputs (a, b); NoNet for plain HMC
//   target(x, E or nullptr, g)           energy and gradient at the chain's temperature
// Exp: lf_update.h's exponential flavour.  Every lane that holds the chain calls this with the same values; the
// callables may be collective.  The callers today are the plain-HMC run and the annealed-importance-sampling run, which
// need neither direction, time nor networks: those are the interface of the two kernels that spell this loop out
// (header), kept so that the three bodies can be read against each other line by line.
template <class Exp, int MD, class Time, class NetX, class NetV, class Target>
__device__ __forceinline__ SmallTraj small_trajectory(int dim, int N, int bwd, float eps, const float* Lm,
                                                      float (&x)[MD], float (&v)[MD], float (&g)[MD], Time time,
                                                      NetX netx, NetV netv, Target target) {
  SmallTraj t;
  float E0, E1;
  target(x, &E0, g);
  float kin0 = 0.f;
#pragma unroll
  for (int d = 0; d < MD; ++d) kin0 += v[d] * v[d];
  t.H0 = E0 + 0.5f * kin0;
  float logdet = 0.f;
  float S[MD], T[MD], Q[MD], bin[MD];
#pragma unroll
  for (int d = 0; d < MD; ++d) S[d] = T[d] = Q[d] = 0.f;
  for (int it = 0; it < N; ++it) {
    const int step = bwd ? N - 1 - it : it;       // utils/dynamics.py:294-296
    float tc, ts;
    time(step, tc, ts);
    const float* m = Lm + step * dim;
    for (int half = 0; half < 2; ++half) {
      if (half == 1) {
        for (int sub = 0; sub < 2; ++sub) {       // keep mask m then 1 - m (fwd) / 1 - m then m (bwd)
          if constexpr (!std::is_same_v<NetX, NoNet<MD>>) {       // (see NoNet)
#pragma unroll
            for (int d = 0; d < MD; ++d) {
              const float k = d < dim ? keep_of(m[d], m[d], bwd, sub) : 1.f;
              bin[d] = k * x[d];
            }
          }
          netx(tc, ts, v, bin, S, T, Q);
#pragma unroll
          for (int d = 0; d < MD; ++d) {
            if (d < dim) {
              float s, omk;
              x[d] = lf_drift<Exp>(x[d], v[d], keep_of(m[d], m[d], bwd, sub), S[d], T[d], Q[d], eps, bwd, s, omk);
              logdet += omk * s;
            }
          }
        }
        target(x, nullptr, g);         // (the energy itself is needed only after the last step: below)
      }
      netv(tc, ts, x, g, S, T, Q);
#pragma unroll
      for (int d = 0; d < MD; ++d) {
        if (d < dim) {
          float s;
          v[d] = lf_kick<Exp>(v[d], g[d], S[d], T[d], Q[d], eps, bwd, s);
          logdet += s;
        }
      }
    }
  }
  target(x, &E1, g);
  float kin1 = 0.f;
#pragma unroll
  for (int d = 0; d < MD; ++d) kin1 += v[d] * v[d];
  t.H1 = E1 + 0.5f * kin1;
  t.logdet = logdet;
  return t;
}

// l2hmc_mix_accept(strict = 0) for one chain (utils/sampler.py:33-59): a forward and a backward value mixed by the
// direction bit (fm = 1 or 0, bm = 1 - fm; plain HMC: fm = 1 and the proposal in both slots), and the
// Metropolis-Hastings decision on element r of stream `stream`
__device__ __forceinline__ float mix_dir(float fm, float bm, float f, float b) { return fm * f + bm * b; }
__device__ __forceinline__ bool mh_accept(float pm, uint64_t seed, uint64_t stream, int64_t r) {
  return pm - philox_uniform_at(seed, stream, r) >= 0.f;
}

}  // namespace l2hmc
