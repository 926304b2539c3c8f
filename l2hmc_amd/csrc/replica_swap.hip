// One replica-exchange (parallel tempering) round between neighbouring rungs of a beta ladder on the 2D U(1) lattice
// (l2hmc_gauge_replica_swap).  Columns [g * group, (g + 1) * group) of x [B][2 T X] are one replica group, column c at
// beta[c]; a round of parity pi proposes the disjoint pairs (a, a + 1), a = g * group + j, j = pi, pi + 2, ... with
// j + 1 < group, and exchanges the two configurations with the Metropolis probability of the joint distribution,
//   p = min(1, exp((beta_a - beta_b) (S_a - S_b))),   S = sum_p (1 - cos P_p)      (accept iff p > u, strict: quirk Q5)
//
// This is the one stage of a ladder run in which chains meet, so it is a launch of its own: the run kernel's workgroups
// never wait for each other (hmc_step.hip), and a pair may sit in two of them.  (Where a whole replica group fits one
// workgroup of 1024 threads, hmc_run_exchange_kernel runs the same round inside the run launch: gauge_swap.h.)
//
// Mapping, chosen for small rows (a pair of 8 x 8 rows is 256 floats): a PAIR is walked by TPP = 64, 128 or 256
// threads -- one wave up to 64 sites, two up to 128, four beyond -- and a workgroup of 256 threads holds 256 / TPP
// pairs.  Thread fl of a pair owns the plaquettes fl, fl + TPP, ... of BOTH rows and reads their four links straight
// from global memory (a row is read 4 times over, from cache; nothing is staged, so nothing caps the lattice size).
// The row sums have ONE order whatever the batch, the group or the parity: a thread adds its plaquettes in ascending
// order, wave_sum adds the lanes of a wave, the waves of the pair are added in ascending order -- S depends on nothing
// but the row (and T, X).  Every thread of the pair then forms p and u itself, and on accept the pair's threads
// exchange the rows element by element (16 bytes per access where the rows allow it).  The barrier between the sums
// and the exchange is also what orders every read of a row ahead of every write to it.
#include "gauge_swap.h"

namespace l2hmc {

constexpr int kSwapThreads = 256;

// S, the decision and the outputs' conventions are gauge_swap.h's, shared with the round inside the run launch
// (hmc_run_exchange_kernel, hmc_step.hip); p is swap_accept_prob (common.h), shared with the toy targets' round too.
// npg: pairs of a group in this round (> 0).  tsh: log2(TPP).  vec: rows are 16-byte aligned and D % 4 == 0.
__global__ __launch_bounds__(kSwapThreads) void replica_swap_kernel(
    float* __restrict__ x, const int T, const int X, const int64_t npairs, const int group, const int parity,
    const int npg, const float* __restrict__ betas, const int64_t chain_stride, const uint64_t seed,
    const uint64_t stream_index, int32_t* __restrict__ replica, float* __restrict__ action,
    float* __restrict__ swap_p, uint8_t* __restrict__ swapped, const int tsh, const int vec) {
  __shared__ float red[kSwapThreads / kWave][2];
  const int tid = threadIdx.x, tpp = 1 << tsh, fl = tid & (tpp - 1), slot = tid >> tsh;
  const int sites = T * X, D = 2 * sites;
  const int64_t pair = (int64_t)blockIdx.x * (kSwapThreads >> tsh) + slot;
  const bool live = pair < npairs;
  const int64_t g = live ? pair / npg : 0;
  const int q = live ? (int)(pair - g * npg) : 0;
  const int j = parity + 2 * q;
  const int64_t a = g * group + j, b = a + 1;
  float* xa = x + a * D;
  float* xb = x + b * D;

  float sa = 0.f, sb = 0.f;
  if (live) {
    for (int s = fl; s < sites; s += tpp) {
      const int i = s / X, jx = s - i * X;
      const int er = 2 * (i * X + (jx + 1 == X ? 0 : jx + 1)), eu = 2 * ((i + 1 == T ? 0 : i + 1) * X + jx) + 1;
      sa += gauge_swap_term(xa[2 * s], xa[2 * s + 1], xa[er], xa[eu]);
      sb += gauge_swap_term(xb[2 * s], xb[2 * s + 1], xb[er], xb[eu]);
    }
  }
  sa = wave_sum(sa);
  sb = wave_sum(sb);
  if ((tid & (kWave - 1)) == 0) {
    red[tid >> 6][0] = sa;
    red[tid >> 6][1] = sb;
  }
  __syncthreads();                       // the sums are published; every plaquette read of the round is behind us
  if (!live) return;
  const int w0 = (slot << tsh) >> 6, nw = tpp >> 6;
  sa = gauge_swap_add_waves(&red[0][0], 2, w0, nw);
  sb = gauge_swap_add_waves(&red[0][1], 2, w0, nw);
  float p;
  const bool acc = gauge_swap_decide(betas[a * chain_stride], betas[b * chain_stride], sa, sb, seed, (uint64_t)a,
                                     stream_index, &p);
  if (fl == 0) {
    if (action) {
      action[a] = sa;
      action[b] = sb;
    }
    gauge_swap_outputs(swap_p, swapped, a, true, p, acc);
    gauge_swap_outputs(swap_p, swapped, b, false, p, acc);
    // the chains of the group that sit the round out: its first at parity 1, its last where one is left over
    if (q == 0 && parity == 1) gauge_swap_outputs(swap_p, swapped, a - 1, false, p, acc);
    if (q == npg - 1 && j + 2 < group) gauge_swap_outputs(swap_p, swapped, b + 1, false, p, acc);
    if (acc && replica) {
      const int32_t t = replica[a];
      replica[a] = replica[b];
      replica[b] = t;
    }
  }
  if (!acc) return;
  if (vec) {
    float4* va = reinterpret_cast<float4*>(xa);
    float4* vb = reinterpret_cast<float4*>(xb);
    for (int i = fl; i < D / 4; i += tpp) {
      const float4 t = va[i];
      va[i] = vb[i];
      vb[i] = t;
    }
  } else {
    for (int i = fl; i < D; i += tpp) {
      const float t = xa[i];
      xa[i] = xb[i];
      xb[i] = t;
    }
  }
}

}  // namespace l2hmc

using namespace l2hmc;

extern "C" int l2hmc_gauge_replica_swap(int32_t T, int32_t X, float* x, int64_t B, int32_t group, int32_t parity,
                                        const float* betas, int64_t chain_stride, uint64_t seed,
                                        uint64_t stream_index, int32_t* replica, float* action, float* swap_p,
                                        uint8_t* swapped, l2hmc_stream_t stream) {
  L2HMC_REQUIRE(T > 0 && X > 0, "gauge_replica_swap: bad lattice T=%d X=%d", T, X);
  L2HMC_REQUIRE((int64_t)T * X <= (1ll << 29), "gauge_replica_swap: lattice %dx%d has more than 2^29 sites", T, X);
  L2HMC_REQUIRE(B >= 0, "gauge_replica_swap: B < 0");
  L2HMC_REQUIRE(group >= 2, "gauge_replica_swap: group = %d: a replica group has 2 rungs or more", group);
  L2HMC_REQUIRE(B % group == 0, "gauge_replica_swap: B = %lld is not a multiple of group = %d", (long long)B, group);
  L2HMC_REQUIRE(parity == 0 || parity == 1, "gauge_replica_swap: parity = %d is not 0 or 1", parity);
  L2HMC_REQUIRE(chain_stride >= 0, "gauge_replica_swap: negative stride");
  if (B == 0) return L2HMC_OK;
  L2HMC_REQUIRE(x && betas, "gauge_replica_swap: NULL x / betas");
  hipStream_t st = (hipStream_t)stream;
  const int npg = (group - parity) / 2;            // j = parity, parity + 2, ... with j + 1 < group
  if (npg == 0) {
    // no pair (group 2 at parity 1): the outputs of a round in which every chain sits out, and no launch
    if (swap_p && hipMemsetAsync(swap_p, 0xff, sizeof(float) * (size_t)B, st) != hipSuccess) {      // all bits set: NaN
      set_error("gauge_replica_swap: %s", hipGetErrorString(hipGetLastError()));
      return L2HMC_ERR_HIP;
    }
    if (swapped && hipMemsetAsync(swapped, 0, (size_t)B, st) != hipSuccess) {
      set_error("gauge_replica_swap: %s", hipGetErrorString(hipGetLastError()));
      return L2HMC_ERR_HIP;
    }
    return L2HMC_OK;
  }
  const int sites = T * X;
  const int tsh = sites <= 64 ? 6 : sites <= 128 ? 7 : 8;
  const int64_t npairs = B / group * npg;
  const int64_t grid = ceil_div(npairs, kSwapThreads >> tsh);
  L2HMC_REQUIRE(grid < (1ll << 31), "gauge_replica_swap: too many pairs");
  // 16-byte accesses: every row starts on a 16-byte boundary (rows are 8 * sites bytes apart)
  const int vec = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && sites % 2 == 0;
  prof_before(kProfSwap, st);
  hipLaunchKernelGGL(replica_swap_kernel, dim3((unsigned)grid), dim3(kSwapThreads), 0, st, x, T, X, npairs, group,
                     parity, npg, betas, chain_stride, seed, stream_index, replica, action, swap_p, swapped, tsh, vec);
  prof_after(kProfSwap, st);
  L2HMC_CHECK_LAUNCH("gauge_replica_swap");
  return L2HMC_OK;
}
