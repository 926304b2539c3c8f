// One replica-exchange (parallel tempering) round between neighbouring rungs of a temperature ladder on a packed toy
// target: the ONE copy of the round, called by small_swap_kernel (l2hmc_small_replica_swap, small_hmc.hip), between
// two MCMC steps of small_hmc_run_kernel<.., EXCHANGE> (l2hmc_small_hmc_run_exchange) and between two steps of
// small_traj_mfma_kernel<.., EXCHANGE> (l2hmc_small_run_exchange, small_mlp.hip).
//
// Geometry: the caller gives every lane its SLOT among the chains its wave holds; slot % G is the rung and the partner
// of a pair sits in lane +- 1.  The callers of small_hmc.hip hold one chain per lane, one wave per workgroup: a
// workgroup holds cpw = (64 / G) * G chains, chain r = blockIdx.x * cpw + lane, slot = lane, so with B % G == 0 and
// G <= 64 a replica group never straddles a wave and both lanes of a pair are live whenever one is; lanes at or beyond
// cpw or B have left the kernel before the first round, which is collective over the rest.  small_traj_mfma_kernel holds chain
// slot = lane & 7 in eight lanes of a wave (cpw = (8 / G) * G, G <= 8): lanes lane and lane +- 1 then hold neighbouring
// chains in the same copy, every copy runs the same round, and the lanes of the idle slots stay in the permutes with
// active = false.
//
// A round of parity pi pairs the columns (a, a + 1), a = g G + j, j = pi, pi + 2, ... with j + 1 < G (the rule of
// l2hmc_gauge_replica_swap); the at most two chains of a group that are in no pair sit the round out (they read their
// own lane).  U is the target's energy at temperature 1 on the lane's fp32 x, formed anew here -- never recovered from
// a step's temperature-scaled E0 / E1 --, so it depends on nothing but the row and the target.  Both lanes of a pair
// form p from the pair's values in (lower, upper) order and u from element a of the stream, so they cannot disagree:
//   p = min(1, exp((1/T_a - 1/T_b) (U_a - U_b)))        (fp64, rounded once; NaN -> 0; exchanged iff p > u, strict: Q5)
// On accept the two lanes trade x[0..dim) and the label by cross-lane reads (ds_bpermute: pairs cross the 16- and
// 32-lane boundaries, which DPP row operations do not); temperature and step size stay with the column.
#pragma once
#include "small_step.h"

namespace l2hmc {

constexpr int kSwapWave = 64;
__host__ __device__ inline int swap_chains_per_wave(int G) { return (kSwapWave / G) * G; }
// pairs of a group in a round of `parity` (j = parity, parity + 2, ... with j + 1 < G)
__host__ __device__ inline int swap_pairs_per_group(int G, int parity) { return (G - parity) / 2; }

// r: the lane's chain; slot: its place among the wave's chains (above); active: false for a lane that holds no chain --
// it proposes nothing and its outputs must be NULL; inv_temp: the 1.f / t the step forms; label: exchanged with x
// (callers without labels pass a dummy).
// (seed, stream): u is element a of what l2hmc_fill_uniform(B, seed, stream) writes.  Outputs, each may be
// NULL, each written by the lane for its own chain r with plain stores -- the chains that sit out included, so nothing
// needs a fill: energy[r] = U for the members of a pair (others untouched), swap_p[r] = p at the lower chain and NaN
// elsewhere, swapped[r] = 1 / 0 at the lower chain and 0 elsewhere.  Returns whether this lane's chain was exchanged.
template <int MD, bool AN>
__device__ __forceinline__ bool small_swap_round(int64_t r, int slot, bool active, int G, int parity, float (&x)[MD],
                                                 float inv_temp,
                                                 int32_t& label, const SmallTarget<MD, AN>& tgt, const float* Lt,
                                                 int dim, int K, const TargetKind& tk, uint64_t seed, uint64_t stream,
                                                 float* energy, float* swap_p, uint8_t* swapped) {
  const float nan = __int_as_float(0x7fc00000);
  if (swap_pairs_per_group(G, parity) == 0) {       // (uniform) group 2 at parity 1: everybody sits out
    if (swap_p) swap_p[r] = nan;
    if (swapped) swapped[r] = 0;
    return false;
  }
  const int lane = (int)threadIdx.x & (kSwapWave - 1), j = slot % G;
  const bool lower = active && j >= parity && ((j - parity) & 1) == 0 && j + 1 < G;
  const bool upper = active && j > parity && ((j - parity) & 1) == 1;
  const int partner = lower ? lane + 1 : upper ? lane - 1 : lane;
  float U, g[MD];
  tgt.eval(Lt, dim, K, tk, 1.f, x, &U, g);
  const float U_o = __shfl(U, partner), it_o = __shfl(inv_temp, partner);
  const float U_a = upper ? U_o : U, U_b = upper ? U : U_o;
  const float it_a = upper ? it_o : inv_temp, it_b = upper ? inv_temp : it_o;
  // exp(-U_b / T_a - U_a / T_b) / exp(-U_a / T_a - U_b / T_b)
  const float p = swap_accept_prob(((double)it_a - (double)it_b) * ((double)U_a - (double)U_b));
  const float u = philox_uniform_at(seed, stream, upper ? r - 1 : r);
  const bool acc = (lower || upper) && p > u;
#pragma unroll
  for (int d = 0; d < MD; ++d) {
    const float xo = __shfl(x[d], partner);
    x[d] = acc ? xo : x[d];
  }
  const int32_t lo = __shfl(label, partner);
  label = acc ? lo : label;
  if (energy && (lower || upper)) energy[r] = U;
  if (swap_p) swap_p[r] = lower ? p : nan;
  if (swapped) swapped[r] = lower && acc ? 1 : 0;
  return acc;
}

}  // namespace l2hmc
