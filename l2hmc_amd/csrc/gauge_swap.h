// The pieces of one replica-exchange round on the 2D U(1) lattice that are part of its bits, held ONCE for the two
// places a round runs: replica_swap_kernel (replica_swap.hip, a launch of its own, rows in global memory) and the round
// inside hmc_run_exchange_kernel (hmc_step.hip, rows in registers and LDS planes).  What the two share: a plaquette's
// term of S, the order in which a row's terms are added (a thread's plaquettes in ascending order, wave_sum over the 64
// lanes, the waves in ascending order), the pairing rule, the decision (fp64 exponent, element a of the uniform
// stream, strict >) and what a chain's outputs hold.  The two paths therefore agree by construction.
#pragma once
#include "fused_step.h"

namespace l2hmc {

// 1 - cos P of one plaquette from its four links (gauge_model.py:676-679: x0[i,j] - x1[i,j] - x0[i,j+1] + x1[i+1,j])
__device__ __forceinline__ float gauge_swap_term(float x0s, float x1s, float x0r, float x1u) {
  const float P = x0s - x1s - x0r + x1u;
  float sn, cs;
  fast_sincos(P, &sn, &cs);
  return 1.f - cs;
}

// wave partials -> the row's S: partials [w0, w0 + nw) (stride floats apart), added in ascending order from 0.f
__device__ __forceinline__ float gauge_swap_add_waves(const float* part, int stride, int w0, int nw) {
  float s = 0.f;
  for (int w = 0; w < nw; ++w) s += part[(w0 + w) * stride];
  return s;
}

// wave_sum of a row that shares its wave with others (tpc = 2^tsh < 64 lanes per row, rows aligned to tpc lanes): the
// row's lanes hold their terms and every other lane 0.f, and adding 0.f is exact, so the row gets the bits wave_sum
// gives it when it sits alone in lanes [0, tpc) of a wave.  Every lane of the wave calls it; returns the sum of the
// calling lane's own row.
__device__ __forceinline__ float gauge_swap_subwave_sum(float v, int tsh) {
  const int sub = (int)(threadIdx.x & (kWave - 1)) >> tsh;
  float mine = 0.f;
  for (int q = 0; q < (kWave >> tsh); ++q) {
    const float t = wave_sum(q == sub ? v : 0.f);
    mine = q == sub ? t : mine;
  }
  return mine;
}

// The place of rung j (column % group) in a round of `parity`: the pairs are (j, j + 1), j = parity, parity + 2, ...
// with j + 1 < group; a rung in no pair sits the round out (group 2 at parity 1: every rung).
__device__ __forceinline__ bool gauge_swap_lower(int j, int group, int parity) {
  return j >= parity && ((j - parity) & 1) == 0 && j + 1 < group;
}
__device__ __forceinline__ bool gauge_swap_upper(int j, int parity) { return j > parity && ((j - parity) & 1) == 1; }

// The decision of the pair (a, a + 1): p = min(1, exp((beta_a - beta_b) (S_a - S_b))) (swap_accept_prob: fp64, rounded
// once, NaN -> 0), u = element a of l2hmc_fill_uniform's stream `stream`, exchanged iff p > u (strict: quirk Q5).
__device__ __forceinline__ bool gauge_swap_decide(float beta_a, float beta_b, float sa, float sb, uint64_t seed,
                                                  uint64_t a, uint64_t stream, float* p) {
  // exp(-beta_b S_a - beta_a S_b) / exp(-beta_a S_a - beta_b S_b)
  *p = swap_accept_prob((double)(beta_a - beta_b) * ((double)sa - (double)sb));
  const float u = philox_u01(seed, a, stream);
  return *p > u;
}

// What a round leaves for chain c (either output may be NULL): p and the decision at the lower chain of a pair, NaN and
// 0 at its upper chain and at a chain that sits out.
__device__ __forceinline__ void gauge_swap_outputs(float* swap_p, uint8_t* swapped, int64_t c, bool lower, float p,
                                                   bool acc) {
  if (swap_p) swap_p[c] = lower ? p : __int_as_float(0x7fc00000);
  if (swapped) swapped[c] = lower && acc ? 1 : 0;
}

}  // namespace l2hmc
