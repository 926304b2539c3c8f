// Annealed importance sampling (AIS, after Wu et al. 2016: utils/ais.py:30-82) on the packed toy targets, a run of
// annealing steps in ONE launch (l2hmc_small_ais_run): the estimator of log(Z1 / Z0), Z = integral of exp(-E), between
// an init Gaussian E0 and the plan's target E1.
//
// Step s of the launch (b_prev = betas[s], b = betas[s + 1]) does, per chain,
//   w += (b - b_prev) (E0(x) - E1(x))             on the state the previous step left (:56-57), in double
//   v  = N(0, I)                                  (:55), or with a persistent momentum v sqrt(1 - rho) + n sqrt(rho) (:53)
//   (Lx, Lv) = one forward plain-HMC trajectory on E_s = (1 - b) E0 + b E1, p = exp(min(0, H_s(x, v) - H_s(Lx, Lv)))
//   accept iff p - u >= 0 (:61): x <- Lx, v <- Lv; else x stays and v <- -Lv, the PROPOSED momentum negated (:63)
//
// The geometry is small_hmc_run_kernel's (small_hmc.hip), for its reasons: a chain without networks is one dependent
// chain of VALU instructions with nothing to share between lanes and nothing for the matrix pipe, so there is one
// THREAD per chain and one wave per workgroup; x, v, the gradient and w stay in the thread's registers from the first
// step to the last; both target images and the masks are staged into LDS once.  The trajectory is small_step.h's with
// NoNet in place of both networks, handed the interpolated energy as its target callable.  E0 and E1 are evaluated by
// SmallTarget, each as its own run instance evaluates it (E1 at the plan's temperature, E0 at temperature 1), and
// combined in float32 as (1.f - b) * E0 + b * E1, the gradient likewise: at b = 1 the step has the bits of
// small_hmc_run_kernel on the plan, at b = 0 those of a run on the init Gaussian.
//
// The weight needs E0 and E1 at the step's start, which the trajectory forms anyway for H_s(x, v): they are taken from
// that evaluation, not formed twice.  The increment and the running sum are double, as small_swap.h forms its
// exponent: a long anneal does not lose its weights to float32 summation, and a run cut into launches, which stores and
// reloads w as the double it is, has the bits of the uncut one.
//
// Draws: two streams per step in the layout of small_hmc_run_kernel -- momenta (or the refresh noise n) elements
// r * dim + d of stream draw0 + 2 s, the Metropolis-Hastings uniform element r of stream draw0 + 2 s + 1.
#include "small_step.h"

namespace l2hmc {

constexpr int kAisThreads = 64;      // one wave: 64 chains per workgroup

struct SmallAisArgs {
  l2hmc_mog_target target, init;     // E1 (any kind, at its temperature), E0 (Gaussian, at temperature 1)
  TargetKind tk;                     // target_kind(target), formed on the host (small_hmc.hip: SmallHmcArgs)
  const float* masks;                // [N][dim]
  int32_t dim, N;
  float eps;
  const float* x_in; float* x_next; int64_t B;
  float* v;                          // [B][dim], read and written, or NULL: fresh momenta every step
  float keep, mix;                   // sqrt(1 - rho), sqrt(rho), formed on the host
  uint64_t seed, draw0;
  int32_t n_steps;
  const float* betas;                // [n_steps + 1]
  double* log_w;                     // [B], read and written
  float* px;                         // [n_steps][B] or NULL
};

// AN: the final target is one of the analytic kinds; the init Gaussian is always the non-analytic form.
template <int MD, bool AN>
__global__ __launch_bounds__(kAisThreads) void small_ais_run_kernel(SmallAisArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int dim = a.dim, N = a.N, K = a.target.K;
  const TargetView tv1 = target_view(dim, K), tv0 = target_view(dim, 1);
  float* Lt1 = lds;
  float* Lt0 = Lt1 + tv1.size;
  float* Lm = Lt0 + tv0.size;                     // masks [N][dim]
  load_target(a.target, Lt1);
  load_target(a.init, Lt0);
  for (int i = threadIdx.x; i < N * dim; i += kAisThreads) Lm[i] = a.masks[i];
  __syncthreads();                                // the only barrier of the kernel

  const int64_t r = (int64_t)blockIdx.x * kAisThreads + threadIdx.x;
  if (r >= a.B) return;                           // chains never meet
  const float eps = a.eps;
  const float inv_temp = 1.f / a.target.temperature;       // the division of small_hmc_run_kernel: its bits at b = 1
  const bool persist = a.v != nullptr;

  float x[MD], v[MD], g[MD], x_init[MD];
#pragma unroll
  for (int d = 0; d < MD; ++d) {
    x[d] = d < dim ? a.x_in[r * dim + d] : 0.f;
    v[d] = (persist && d < dim) ? a.v[r * dim + d] : 0.f;
  }
  double w = a.log_w[r];
  SmallTarget<MD, AN> t1;
  SmallTarget<MD, false> t0;
  const TargetKind tk1 = a.tk;
  TargetKind tk0;
  tk0.kind = L2HMC_TARGET_GAUSSIAN;
  tk0.eps = tk0.a = 1.f;
  t1.load(Lt1, dim, K);
  t0.load(Lt0, dim, 1);

  float b = 0.f, omb = 1.f;                       // of the step
  float e0_start = 0.f, e1_start = 0.f;           // E0, E1 at the step's start
  bool at_start = false;
  auto target = [&](const float (&xx)[MD], float* E, float (&gg)[MD]) __attribute__((always_inline)) {
    float g0[MD], g1[MD], e0 = 0.f, e1 = 0.f;
    t0.eval(Lt0, dim, 1, tk0, 1.f, xx, E ? &e0 : nullptr, g0);
    t1.eval(Lt1, dim, K, tk1, inv_temp, xx, E ? &e1 : nullptr, g1);
#pragma unroll
    for (int d = 0; d < MD; ++d) gg[d] = omb * g0[d] + b * g1[d];
    if (E) {
      *E = omb * e0 + b * e1;
      if (at_start) {                             // (the trajectory's first call: folded once it is inlined)
        e0_start = e0;
        e1_start = e1;
        at_start = false;
      }
    }
  };
  auto no_time = [](int, float& tc, float& ts) __attribute__((always_inline)) { tc = ts = 0.f; };

  for (int sidx = 0; sidx < a.n_steps; ++sidx) {
    const uint64_t draw = a.draw0 + 2 * (uint64_t)sidx;
    const float b_prev = a.betas[sidx];
    b = a.betas[sidx + 1];
    omb = 1.f - b;
    // momenta or refresh noise: elements r * dim + d of stream `draw`, a Philox block for four of them
    {
      float nv[4] = {0.f, 0.f, 0.f, 0.f};
      int64_t have = -1;
#pragma unroll
      for (int d = 0; d < MD; ++d) {
        if (d < dim) {
          const int64_t i = r * dim + d;
          if ((i >> 2) != have) {
            uint32_t c[4];
            philox_block_at(a.seed, draw, i, c);
            philox_normal4(c, nv);
            have = i >> 2;
          }
          const int j = (int)(i & 3);
          const float n = j == 0 ? nv[0] : j == 1 ? nv[1] : j == 2 ? nv[2] : nv[3];
          v[d] = persist ? v[d] * a.keep + n * a.mix : n;
        } else {
          v[d] = 0.f;
        }
      }
    }
#pragma unroll
    for (int d = 0; d < MD; ++d) x_init[d] = x[d];
    at_start = true;
    const SmallTraj tj =
        small_trajectory<ExpFast>(dim, N, 0, eps, Lm, x, v, g, no_time, NoNet<MD>{}, NoNet<MD>{}, target);
    w += ((double)b - (double)b_prev) * ((double)e0_start - (double)e1_start);
    const float pacc = tj.p_accept();
    const bool acc = mh_accept(pacc, a.seed, draw + 1, r);
    if (a.px) a.px[(int64_t)sidx * a.B + r] = pacc;
#pragma unroll
    for (int d = 0; d < MD; ++d) {
      x[d] = acc ? x[d] : x_init[d];
      v[d] = acc ? v[d] : -v[d];                  // the proposed momentum, negated (utils/ais.py:63)
    }
  }
  a.log_w[r] = w;
#pragma unroll
  for (int d = 0; d < MD; ++d) {
    if (d < dim) {
      a.x_next[r * dim + d] = x[d];
      if (persist) a.v[r * dim + d] = v[d];
    }
  }
}

template <int MD>
static int launch_small_ais(const SmallAisArgs& a, size_t lds, hipStream_t st) {
  const dim3 grid((unsigned)ceil_div(a.B, kAisThreads));
  prof_before(kProfSmall, st);
  if (target_is_analytic(a.target.is_gaussian))
    hipLaunchKernelGGL((small_ais_run_kernel<MD, true>), grid, dim3(kAisThreads), lds, st, a);
  else
    hipLaunchKernelGGL((small_ais_run_kernel<MD, false>), grid, dim3(kAisThreads), lds, st, a);
  prof_after(kProfSmall, st);
  L2HMC_CHECK_LAUNCH("small_ais_run");
  return L2HMC_OK;
}

}  // namespace l2hmc

using namespace l2hmc;

// Every check comes before any device call.  (The schedule, the weights and the momenta live on the device and are not
// looked at.)
extern "C" int l2hmc_small_ais_run(const l2hmc_small_plan* plan, const l2hmc_mog_target* init, const float* x_in,
                                   float* x_next, float* v, float refreshment, int64_t B, uint64_t seed,
                                   uint64_t draw0, int32_t n_steps, const float* betas, double* log_w, float* px,
                                   l2hmc_stream_t stream) {
  const char* who = "small_ais_run";
  if (int e = check_small_run_args(who, plan, x_in, x_next, B, draw0, n_steps, 2, 0, 0)) return e;
  L2HMC_REQUIRE(init != nullptr, "%s: init is NULL", who);
  L2HMC_REQUIRE(betas != nullptr && log_w != nullptr, "%s: betas / log_w is NULL", who);
  L2HMC_REQUIRE(plan->hmc, "%s: the plan is an L2HMC sampler's (hmc == 0): the anneal runs plain-HMC transitions", who);
  if (int e = check_small_plan(plan, who, false)) return e;
  L2HMC_REQUIRE(init->is_gaussian == L2HMC_TARGET_GAUSSIAN && init->dim == plan->x_dim,
                "%s: init is a target of kind %d and dim=%d: expected a Gaussian (kind %d) of dim=%d", who,
                init->is_gaussian, init->dim, L2HMC_TARGET_GAUSSIAN, plan->x_dim);
  l2hmc_mog_target init1 = *init;
  init1.temperature = 1.f;                        // evaluated at temperature 1 whatever its field says
  if (int e = check_target_args(&init1, "small_ais_run: init")) return e;
  L2HMC_REQUIRE(v == nullptr || (refreshment > 0.f && refreshment <= 1.f),
                "%s: refreshment = %g is not in (0, 1] (v is given: the momentum persists)", who, (double)refreshment);
  const int dim = plan->x_dim, N = plan->trajectory_length;
  const size_t lds = sizeof(float) * ((size_t)target_view(dim, plan->target.K).size + (size_t)target_view(dim, 1).size +
                                      (size_t)N * dim);
  L2HMC_REQUIRE(lds <= 64 * 1024, "%s: trajectory_length=%d: targets and masks take %zu B of LDS (max 65536)", who, N,
                lds);
  if (B == 0) return L2HMC_OK;
  L2HMC_REQUIRE(ceil_div(B, kAisThreads) < (1ll << 31), "%s: too many chains", who);
  SmallAisArgs a{};
  a.target = plan->target; a.init = init1; a.tk = target_kind(plan->target); a.masks = plan->masks;
  a.dim = dim; a.N = N; a.eps = plan->eps;
  a.x_in = x_in; a.x_next = x_next; a.B = B; a.v = v;
  a.keep = v ? sqrtf(1.f - refreshment) : 0.f; a.mix = v ? sqrtf(refreshment) : 1.f;
  a.seed = seed; a.draw0 = draw0; a.n_steps = n_steps; a.betas = betas; a.log_w = log_w; a.px = px;
  hipStream_t st = (hipStream_t)stream;
  return dim <= 2 ? launch_small_ais<2>(a, lds, st) : launch_small_ais<kMaxDim>(a, lds, st);
}
