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
#include "small_step.h"

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

// TEMPERED: a template flag for the reason given at small_traj_mfma_kernel -- the untempered instances hold
// 1 / temperature for the launch and keep their code.
template <int MD, bool AN, bool TEMPERED>
__global__ __launch_bounds__(kHmcThreads) void small_hmc_run_kernel(SmallHmcArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int dim = a.dim, N = a.N, K = a.target.K;
  const TargetView tv = target_view(a.target.dim, K);
  float* Lt = lds;
  float* Lm = Lt + tv.size;                       // masks [N][dim]
  load_target(a.target, Lt);
  for (int i = threadIdx.x; i < N * dim; i += kHmcThreads) Lm[i] = a.masks[i];
  __syncthreads();                                // the only barrier of the kernel

  const int64_t r = (int64_t)blockIdx.x * kHmcThreads + threadIdx.x;
  if (r >= a.B) return;                           // chains never meet: nothing below is collective
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

  for (int sidx = 0; sidx < a.n_steps; ++sidx) {
    const uint64_t draw = a.draw0 + 2 * (uint64_t)sidx;
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
