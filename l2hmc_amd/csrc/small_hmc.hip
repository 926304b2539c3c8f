// Plain HMC on the packed toy targets, a run of MCMC steps in ONE launch (l2hmc_small_hmc_run): the baseline every
// L2HMC figure is compared against (utils/dynamics.py:75-78 -- both networks return zeros --, utils/sampler.py:30-32,
// :57-59).
//
// One THREAD per chain, one wave per workgroup.  A chain without networks is a few dozen dependent VALU instructions
// per leapfrog step: nothing to share between lanes, nothing for the matrix pipe, and a launch of 128..4096 chains is
// bound by the latency of that one dependent chain.  So x, v and the gradient (x_dim <= 8) stay in the thread's
// registers from the first step to the last, the target and the masks are staged into LDS once per workgroup, and
// workgroups of 64 chains spread a batch over as many compute units as it has waves.  small_traj_mfma_kernel
// (small_mlp.hip), which the loop over `propose` runs for an hmc plan, gives a chain four lanes, 16 chains a wave of
// 256-thread workgroups and sizes its LDS image for two networks that are not there.
//
// The arithmetic is small_step.h's: the trajectory small_traj_mfma_kernel runs for an hmc plan, here with NoNet in
// place of both networks (S = T = Q = 0, which the compiler folds), on the same target instances (MD = 2 for
// x_dim <= 2, kMaxDim otherwise; AN for the analytic kinds), followed by mix_accept_kernel(strict = 0) as sampler.py's
// tf_accept calls it, so a run gives the bits of the loop over fill_normal, l2hmc_small_trajectory, fill_uniform and
// l2hmc_mix_accept.
//
// Also here, because they share that mapping: the run with replica exchange between the columns of a temperature
// ladder inside the launch (l2hmc_small_hmc_run_exchange, the EXCHANGE instances of the run kernel) and one round on its
// own (l2hmc_small_replica_swap, small_swap_kernel); the round itself is small_swap.h's.
#include "small_swap.h"

namespace l2hmc {

constexpr int kHmcThreads = 64;      // one wave: 64 chains per workgroup

struct SmallHmcArgs {
  l2hmc_mog_target target;
  // target_kind(target), formed on the host: read in the kernel, the rough well's scalars in the union slot of `mu`
  // put the whole argument block on the stack (16 B of scratch per lane in the analytic instances)
  TargetKind tk;
  const float* masks;                // [N][dim]
  int32_t dim, N;
  float eps;
  const float* eps_chain;            // [B] or NULL (eps for every chain)
  const float* x_in; float* x_next; int64_t B;
  uint64_t seed, draw0;
  int32_t n_steps;
  // TEMPERED instance: step s of chain c runs at temps[s * temp_step_stride + c * temp_chain_stride]
  const float* temps; int64_t temp_step_stride, temp_chain_stride;
  float* px; float* samples;         // [n_steps][B], [n_steps][B][dim]; each may be NULL
};

// What the EXCHANGE instances take on top: a replica-exchange round (small_swap.h) after step s of the launch iff
// (swap_phase + s + 1) % swap_every == 0, the j-th of them with parity (first_parity + j) % 2.  A struct of its own, as
// HmcLadderArgs is (hmc_step.hip): SmallHmcArgs sits on the stack in the analytic instances and does not grow, and
// the instances without exchange keep their kernel arguments.
struct SmallHmcExchangeArgs : SmallHmcArgs {
  int32_t group, swap_every, swap_phase, first_parity;
  int32_t* replica;                  // [B] labels, read on entry and written on exit, or NULL
  float* swap_p; uint8_t* swapped; int32_t* replica_hist;      // [rounds][B]; each may be NULL
};

// TEMPERED: a template flag for the reason given at small_traj_mfma_kernel -- the untempered instances hold
// 1 / temperature for the launch and keep their code.
// EXCHANGE (always TEMPERED): the rungs of a replica group sit in ONE wave (small_swap.h: cpw chains per workgroup
// instead of 64), so a round is a handful of cross-lane reads between two steps of chains that stay in registers -- no
// barrier, no workspace, no launch.  Streams in the order of the loop a caller would write: two per step, the next one
// per round (a round without a pair takes its stream as well).
template <int MD, bool AN, bool TEMPERED, bool EXCHANGE = false>
__global__ __launch_bounds__(kHmcThreads) void small_hmc_run_kernel(
    std::conditional_t<EXCHANGE, SmallHmcExchangeArgs, SmallHmcArgs> a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int dim = a.dim, N = a.N, K = a.target.K;
  const TargetView tv = target_view(a.target.dim, K);
  float* Lt = lds;
  float* Lm = Lt + tv.size;                       // masks [N][dim]
  load_target(a.target, Lt);
  for (int i = threadIdx.x; i < N * dim; i += kHmcThreads) Lm[i] = a.masks[i];
  __syncthreads();                                // the only barrier of the kernel

  int cpw = kHmcThreads;                          // chains of this workgroup
  if constexpr (EXCHANGE) cpw = swap_chains_per_wave(a.group);
  const int64_t r = (int64_t)blockIdx.x * cpw + threadIdx.x;
  // chains never meet, or (EXCHANGE) meet within their group, whose lanes all stay: B % group == 0
  if (r >= a.B || (EXCHANGE && (int)threadIdx.x >= cpw)) return;
  const float eps = a.eps_chain ? a.eps_chain[r] : a.eps;
  float inv_temp = TEMPERED ? 1.f : 1.f / a.target.temperature;      // (TEMPERED: set at the head of every step)

  float x[MD], v[MD], g[MD], x_init[MD];
#pragma unroll
  for (int d = 0; d < MD; ++d) x[d] = d < dim ? a.x_in[r * dim + d] : 0.f;
  SmallTarget<MD, AN> tgt;
  const TargetKind tk = a.tk;
  tgt.load(Lt, dim, K);
  auto target = [&](const float (&xx)[MD], float* E, float (&gg)[MD]) __attribute__((always_inline)) {
    tgt.eval(Lt, dim, K, tk, inv_temp, xx, E, gg);
  };
  auto no_time = [](int, float& tc, float& ts) __attribute__((always_inline)) { tc = ts = 0.f; };

  // EXCHANGE: the label that travels with x, the next stream, the steps until the next round and that round's index
  [[maybe_unused]] int32_t label = 0;
  [[maybe_unused]] uint64_t next = a.draw0;
  [[maybe_unused]] int until = 0, round = 0;
  if constexpr (EXCHANGE) {
    if (a.replica) label = a.replica[r];
    until = a.swap_every - a.swap_phase;
  }

  for (int sidx = 0; sidx < a.n_steps; ++sidx) {
    const uint64_t draw = EXCHANGE ? next : a.draw0 + 2 * (uint64_t)sidx;
    // the same division as above, so equal temperatures give equal bits; one temperature from E0 to E1
    if constexpr (TEMPERED) inv_temp = 1.f / a.temps[(int64_t)sidx * a.temp_step_stride + r * a.temp_chain_stride];
    // momenta: elements r * dim + d of stream `draw`.  A Philox block holds four of them, so consecutive components
    // mostly share one
    {
      float nv[4] = {0.f, 0.f, 0.f, 0.f};
      int64_t have = -1;
#pragma unroll
      for (int d = 0; d < MD; ++d) {
        v[d] = 0.f;
        if (d < dim) {
          const int64_t i = r * dim + d;
          if ((i >> 2) != have) {
            uint32_t c[4];
            philox_block_at(a.seed, draw, i, c);
            philox_normal4(c, nv);
            have = i >> 2;
          }
          const int j = (int)(i & 3);
          v[d] = j == 0 ? nv[0] : j == 1 ? nv[1] : j == 2 ? nv[2] : nv[3];
        }
      }
    }
#pragma unroll
    for (int d = 0; d < MD; ++d) x_init[d] = x[d];
    const SmallTraj tj =
        small_trajectory<ExpFast>(dim, N, 0, eps, Lm, x, v, g, no_time, NoNet<MD>{}, NoNet<MD>{}, target);
    const float pacc = tj.p_accept();
    // mix_accept_kernel(strict = 0) with coin = 1 and the proposal in both slots (sampler.py: tf_accept)
    const float fm = 1.f, bm = 1.f - fm;
    const float pm = mix_dir(fm, bm, pacc, pacc);
    const bool acc = mh_accept(pm, a.seed, draw + 1, r);
    if (a.px) a.px[(int64_t)sidx * a.B + r] = pm;
#pragma unroll
    for (int d = 0; d < MD; ++d) {
      const float xp = mix_dir(fm, bm, x[d], x[d]);
      x[d] = acc ? xp : x_init[d];
      if (a.samples && d < dim) a.samples[((int64_t)sidx * a.B + r) * dim + d] = x[d];
    }
    if constexpr (EXCHANGE) {
      next += 2;
      if (--until == 0) {                         // (uniform) on the state and at the temperatures of this step
        const int64_t row = (int64_t)round * a.B;
        small_swap_round<MD, AN>(r, (int)threadIdx.x, true, a.group, (a.first_parity + round) & 1, x, inv_temp, label,
                                 tgt, Lt, dim, K, tk, a.seed, next, nullptr, a.swap_p ? a.swap_p + row : nullptr,
                                 a.swapped ? a.swapped + row : nullptr);
        if (a.replica_hist) a.replica_hist[row + r] = label;
        next += 1;
        ++round;
        until = a.swap_every;
      }
    }
  }
  if constexpr (EXCHANGE) {
    if (a.replica) a.replica[r] = label;
  }
#pragma unroll
  for (int d = 0; d < MD; ++d)
    if (d < dim) a.x_next[r * dim + d] = x[d];
}

template <int MD, bool AN, bool TEMPERED>
static int launch_small_hmc(const SmallHmcArgs& a, size_t lds, hipStream_t st) {
  const dim3 grid((unsigned)ceil_div(a.B, kHmcThreads));
  prof_before(kProfSmall, st);
  hipLaunchKernelGGL((small_hmc_run_kernel<MD, AN, TEMPERED>), grid, dim3(kHmcThreads), lds, st, a);
  prof_after(kProfSmall, st);
  L2HMC_CHECK_LAUNCH("small_hmc_run");
  return L2HMC_OK;
}

template <int MD>
static int launch_small_hmc_exchange(const SmallHmcExchangeArgs& a, size_t lds, hipStream_t st) {
  const dim3 grid((unsigned)ceil_div(a.B, swap_chains_per_wave(a.group)));
  prof_before(kProfSmall, st);
  if (target_is_analytic(a.target.is_gaussian))
    hipLaunchKernelGGL((small_hmc_run_kernel<MD, true, true, true>), grid, dim3(kHmcThreads), lds, st, a);
  else
    hipLaunchKernelGGL((small_hmc_run_kernel<MD, false, true, true>), grid, dim3(kHmcThreads), lds, st, a);
  prof_after(kProfSmall, st);
  L2HMC_CHECK_LAUNCH("small_hmc_run_exchange");
  return L2HMC_OK;
}

// ONE round on its own (l2hmc_small_replica_swap): the geometry of the exchange instances above, the chain read from
// and, where it was exchanged, written back to global memory.
template <int MD, bool AN>
__global__ __launch_bounds__(kHmcThreads) void small_swap_kernel(
    const l2hmc_mog_target target, const TargetKind tk, float* __restrict__ xg, const int64_t B, const int group,
    const int parity, const float* __restrict__ temps, const int64_t chain_stride, const uint64_t seed,
    const uint64_t stream_index, int32_t* __restrict__ replica, float* __restrict__ energy,
    float* __restrict__ swap_p, uint8_t* __restrict__ swapped) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int dim = target.dim, K = target.K;
  load_target(target, lds);
  __syncthreads();
  const int cpw = swap_chains_per_wave(group);
  const int64_t r = (int64_t)blockIdx.x * cpw + threadIdx.x;
  if (r >= B || (int)threadIdx.x >= cpw) return;
  float x[MD];
#pragma unroll
  for (int d = 0; d < MD; ++d) x[d] = d < dim ? xg[r * dim + d] : 0.f;
  const float inv_temp = 1.f / temps[r * chain_stride];
  int32_t label = replica ? replica[r] : 0;
  SmallTarget<MD, AN> tgt;
  tgt.load(lds, dim, K);
  if (!small_swap_round<MD, AN>(r, (int)threadIdx.x, true, group, parity, x, inv_temp, label, tgt, lds, dim, K, tk,
                                seed, stream_index, energy, swap_p, swapped))
    return;
#pragma unroll
  for (int d = 0; d < MD; ++d)
    if (d < dim) xg[r * dim + d] = x[d];
  if (replica) replica[r] = label;
}

template <int MD>
static int launch_small_hmc_md(const SmallHmcArgs& a, size_t lds, hipStream_t st) {
  const bool an = target_is_analytic(a.target.is_gaussian);
  if (a.temps) return an ? launch_small_hmc<MD, true, true>(a, lds, st) : launch_small_hmc<MD, false, true>(a, lds, st);
  return an ? launch_small_hmc<MD, true, false>(a, lds, st) : launch_small_hmc<MD, false, false>(a, lds, st);
}

}  // namespace l2hmc

using namespace l2hmc;

// Every check comes before any device call.  (Temperatures and step sizes live on the device and are not looked at.)
extern "C" int l2hmc_small_hmc_run(const l2hmc_small_plan* plan, const float* x_in, float* x_next, int64_t B,
                                   uint64_t seed, uint64_t draw0, int32_t n_steps, const float* temps,
                                   int64_t step_stride, int64_t chain_stride, const float* eps_chain, float* px,
                                   float* samples, l2hmc_stream_t stream) {
  const char* who = "small_hmc_run";
  if (int e = check_small_run_args(who, plan, x_in, x_next, B, draw0, n_steps, 2, step_stride, chain_stride)) return e;
  L2HMC_REQUIRE(plan->hmc, "small_hmc_run: the plan is an L2HMC sampler's (hmc == 0), which proposes in both "
                           "directions with its networks: use l2hmc_small_run");
  if (int e = check_small_plan(plan, who, false)) return e;
  const int dim = plan->x_dim, N = plan->trajectory_length;
  const size_t lds = sizeof(float) * ((size_t)target_view(dim, plan->target.K).size + (size_t)N * dim);
  L2HMC_REQUIRE(lds <= 64 * 1024, "small_hmc_run: trajectory_length=%d: target and masks take %zu B of LDS (max 65536)",
                N, lds);
  if (B == 0) return L2HMC_OK;
  SmallHmcArgs a{};
  a.target = plan->target; a.tk = target_kind(plan->target); a.masks = plan->masks; a.dim = dim; a.N = N; a.eps = plan->eps; a.eps_chain = eps_chain;
  a.x_in = x_in; a.x_next = x_next; a.B = B; a.seed = seed; a.draw0 = draw0; a.n_steps = n_steps;
  a.temps = temps; a.temp_step_stride = step_stride; a.temp_chain_stride = chain_stride;
  a.px = px; a.samples = samples;
  hipStream_t st = (hipStream_t)stream;
  return dim <= 2 ? launch_small_hmc_md<2>(a, lds, st) : launch_small_hmc_md<kMaxDim>(a, lds, st);
}

// What both replica-exchange entries check of a group
static int check_small_group(const char* who, int64_t B, int32_t group) {
  L2HMC_REQUIRE(group >= 2 && group <= kSwapWave,
                "%s: group = %d: a replica group has 2 rungs or more and sits in one wave (at most %d)", who, group,
                kSwapWave);
  L2HMC_REQUIRE(B % group == 0, "%s: B = %lld is not a multiple of group = %d", who, (long long)B, group);
  return L2HMC_OK;
}

extern "C" int l2hmc_small_replica_swap(const l2hmc_small_plan* plan, float* x, int64_t B, int32_t group,
                                        int32_t parity, const float* temps, int64_t chain_stride, uint64_t seed,
                                        uint64_t stream_index, int32_t* replica, float* energy, float* swap_p,
                                        uint8_t* swapped, l2hmc_stream_t stream) {
  const char* who = "small_replica_swap";
  L2HMC_REQUIRE(plan != nullptr, "%s: plan is NULL", who);
  L2HMC_REQUIRE(B >= 0, "%s: B < 0", who);
  if (int e = check_small_group(who, B, group)) return e;
  L2HMC_REQUIRE(parity == 0 || parity == 1, "%s: parity = %d is not 0 or 1", who, parity);
  L2HMC_REQUIRE(chain_stride >= 0, "%s: negative stride", who);
  // of the plan only x_dim and the target are read: an L2HMC sampler's plan is served as a plain-HMC one is
  L2HMC_REQUIRE(plan->x_dim == plan->target.dim, "%s: x_dim=%d != target dim=%d", who, plan->x_dim, plan->target.dim);
  if (int e = check_target_args(&plan->target, who)) return e;
  if (B == 0) return L2HMC_OK;
  L2HMC_REQUIRE(x && temps, "%s: NULL x / temps", who);
  hipStream_t st = (hipStream_t)stream;
  if (swap_pairs_per_group(group, parity) == 0) {
    // no pair (group 2 at parity 1): the outputs of a round in which every chain sits out, and no launch
    if (swap_p && hipMemsetAsync(swap_p, 0xff, sizeof(float) * (size_t)B, st) != hipSuccess) {      // all bits set: NaN
      set_error("%s: %s", who, hipGetErrorString(hipGetLastError()));
      return L2HMC_ERR_HIP;
    }
    if (swapped && hipMemsetAsync(swapped, 0, (size_t)B, st) != hipSuccess) {
      set_error("%s: %s", who, hipGetErrorString(hipGetLastError()));
      return L2HMC_ERR_HIP;
    }
    return L2HMC_OK;
  }
  const l2hmc_mog_target& t = plan->target;
  const int64_t grid = ceil_div(B, swap_chains_per_wave(group));
  L2HMC_REQUIRE(grid < (1ll << 31), "%s: too many chains", who);
  const size_t lds = sizeof(float) * (size_t)target_view(t.dim, t.K).size;
  const TargetKind tk = target_kind(t);
  const bool an = target_is_analytic(t.is_gaussian);
  const dim3 g((unsigned)grid), b(kHmcThreads);
  prof_before(kProfSwap, st);
#define L2HMC_SWAP_LAUNCH(MD, AN)                                                                                   \
  hipLaunchKernelGGL((small_swap_kernel<MD, AN>), g, b, lds, st, t, tk, x, B, group, parity, temps, chain_stride,   \
                     seed, stream_index, replica, energy, swap_p, swapped)
  if (t.dim <= 2) {
    if (an) L2HMC_SWAP_LAUNCH(2, true); else L2HMC_SWAP_LAUNCH(2, false);
  } else {
    if (an) L2HMC_SWAP_LAUNCH(kMaxDim, true); else L2HMC_SWAP_LAUNCH(kMaxDim, false);
  }
#undef L2HMC_SWAP_LAUNCH
  prof_after(kProfSwap, st);
  L2HMC_CHECK_LAUNCH(who);
  return L2HMC_OK;
}

extern "C" int l2hmc_small_hmc_run_exchange(const l2hmc_small_plan* plan, const float* x_in, float* x_next, int64_t B,
                                            uint64_t seed, uint64_t draw0, int32_t n_steps, const float* temps,
                                            int64_t step_stride, int64_t chain_stride, const float* eps_chain,
                                            int32_t group, int32_t swap_every, int32_t swap_phase,
                                            int32_t first_parity, int32_t* replica, float* px, float* samples,
                                            float* swap_p, uint8_t* swapped, int32_t* replica_hist,
                                            l2hmc_stream_t stream) {
  const char* who = "small_hmc_run_exchange";
  if (int e = check_small_run_args(who, plan, x_in, x_next, B, draw0, n_steps, 2, step_stride, chain_stride)) return e;
  L2HMC_REQUIRE(plan->hmc, "%s: the plan is an L2HMC sampler's (hmc == 0): its exchange run is "
                           "l2hmc_small_run_exchange", who);
  if (int e = check_small_plan(plan, who, false)) return e;
  L2HMC_REQUIRE(temps != nullptr, "%s: temps is NULL (a replica group is a ladder of temperatures)", who);
  if (int e = check_small_group(who, B, group)) return e;
  L2HMC_REQUIRE(swap_every >= 1, "%s: swap_every = %d must be 1 or more", who, swap_every);
  L2HMC_REQUIRE(swap_phase >= 0 && swap_phase < swap_every, "%s: swap_phase = %d is not in [0, swap_every = %d)", who,
                swap_phase, swap_every);
  L2HMC_REQUIRE(first_parity == 0 || first_parity == 1, "%s: first_parity = %d is not 0 or 1", who, first_parity);
  // a round after step s iff (swap_phase + s + 1) % swap_every == 0
  const uint64_t rounds = ((uint64_t)swap_phase + (uint64_t)n_steps) / (uint64_t)swap_every;
  L2HMC_REQUIRE(rounds <= UINT64_MAX - draw0 - 2 * (uint64_t)n_steps,
                "%s: draw0 + 2 * n_steps + rounds overflows 64 bits (draw0=%llu, n_steps=%d, rounds=%llu)", who,
                (unsigned long long)draw0, n_steps, (unsigned long long)rounds);
  const int dim = plan->x_dim, N = plan->trajectory_length;
  const size_t lds = sizeof(float) * ((size_t)target_view(dim, plan->target.K).size + (size_t)N * dim);
  L2HMC_REQUIRE(lds <= 64 * 1024, "%s: trajectory_length=%d: target and masks take %zu B of LDS (max 65536)", who, N,
                lds);
  if (B == 0) return L2HMC_OK;
  L2HMC_REQUIRE(ceil_div(B, swap_chains_per_wave(group)) < (1ll << 31), "%s: too many chains", who);
  SmallHmcExchangeArgs a{};
  a.target = plan->target; a.tk = target_kind(plan->target); a.masks = plan->masks; a.dim = dim; a.N = N; a.eps = plan->eps; a.eps_chain = eps_chain;
  a.x_in = x_in; a.x_next = x_next; a.B = B; a.seed = seed; a.draw0 = draw0; a.n_steps = n_steps;
  a.temps = temps; a.temp_step_stride = step_stride; a.temp_chain_stride = chain_stride;
  a.px = px; a.samples = samples;
  a.group = group; a.swap_every = swap_every; a.swap_phase = swap_phase; a.first_parity = first_parity;
  a.replica = replica; a.swap_p = swap_p; a.swapped = swapped; a.replica_hist = replica_hist;
  hipStream_t st = (hipStream_t)stream;
  return dim <= 2 ? launch_small_hmc_exchange<2>(a, lds, st) : launch_small_hmc_exchange<kMaxDim>(a, lds, st);
}
