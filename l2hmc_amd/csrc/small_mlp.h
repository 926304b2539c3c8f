// Device and host helpers shared by the toy-target integrator (small_mlp.hip), its training kernel (small_train.hip)
// and the plain-HMC run (small_hmc.hip): LDS images of the MLP weights and the mixture target, the ONE network
// evaluation by the sixteen lanes of a chain (the training kernel's forward and reverse passes), closed-form energy /
// gradient (from LDS, and from registers: TargetRegs), single elements of the library's Philox streams, and the host
// checks of a plan, its networks and a run's arguments that every entry makes before any launch.  The stages of a
// sampler step built from these: small_step.h.
#pragma once
#include "common.h"


namespace l2hmc {

constexpr int kSmallThreads = 256;   // 16 chains per workgroup
constexpr int kLPC = 16;              // lanes per chain
constexpr int kMaxDim = L2HMC_MAX_SMALL_DIM;
constexpr int kMaxMix = L2HMC_MAX_MIX;

struct SmallNetView {   // offsets (floats) into the per-net LDS image; weight matrices are k-major [k][HP]
  int w1, wt, b1, wh, bh, whd, bhd, es, eq, size;
};

__host__ __device__ inline SmallNetView small_net_view(int HP, int dim) {
  SmallNetView v;
  int o = 0;
  v.w1 = o; o += 2 * dim * HP;      // [2*dim][HP]
  v.wt = o; o += 2 * HP;            // [2][HP]
  v.b1 = o; o += HP;
  v.wh = o; o += HP * HP;           // [k][n]
  v.bh = o; o += HP;
  v.whd = o; o += 3 * dim * HP;     // [3*dim][k]
  v.bhd = o; o += 3 * dim;
  v.es = o; o += dim;
  v.eq = o; o += dim;
  v.size = (o + 3) & ~3;
  return v;
}

template <int HP>
__device__ void load_net(const l2hmc_dense_net& n, float* L, int dim) {
  const SmallNetView v = small_net_view(HP, dim);
  const int H = n.H, tid = threadIdx.x;
  for (int i = tid; i < v.size; i += blockDim.x) L[i] = 0.f;
  __syncthreads();
  // packed global layouts: w1_t [H][2*dim], wh_t [H (out)][H (in)], whd_t [3][dim][H]
  for (int i = tid; i < H * 2 * dim; i += blockDim.x) L[v.w1 + (i % (2 * dim)) * HP + i / (2 * dim)] = n.w1_t[i];
  for (int i = tid; i < 2 * H; i += blockDim.x) L[v.wt + (i / H) * HP + (i % H)] = n.wt[i];
  for (int i = tid; i < H; i += blockDim.x) {
    L[v.b1 + i] = n.b1[i];
    L[v.bh + i] = n.bh[i];
  }
  for (int i = tid; i < H * H; i += blockDim.x) L[v.wh + (i % H) * HP + i / H] = n.wh_t[i];
  for (int i = tid; i < 3 * dim * H; i += blockDim.x) L[v.whd + (i / H) * HP + (i % H)] = n.whd_t[i];
  for (int i = tid; i < 3 * dim; i += blockDim.x) L[v.bhd + i] = n.bhd[i];
  for (int i = tid; i < dim; i += blockDim.x) {
    L[v.es + i] = expf(n.coeff_s[i]);
    L[v.eq + i] = expf(n.coeff_q[i]);
  }
}

// (S, T, Q) = net([a, b, t]) for the chain this lane belongs to.  `sub` = lane within the chain (0..15),
// `hrow` = the chain's HP-float LDS row for the hidden-vector exchange.  Must be called by all threads of the
// workgroup (it contains workgroup barriers).  h1 / h2 [HP / 16]: this lane's hidden units after the relu, which the
// training kernel's reverse pass differentiates through (its forward pass drops them).
// MD: compile-time bound on x_dim (2 for the benchmark targets, kMaxDim otherwise); register arrays and the
// unrolled loops are sized by it.
template <int HP, int MD = L2HMC_MAX_SMALL_DIM>
__device__ void net_eval(const float* L, int dim, int q_tanh, const float* a, const float* b, float tc, float ts,
                         int sub, float* hrow, float* h1, float* h2, float* S, float* T, float* Q) {
  constexpr int kMaxDim = MD;
  constexpr int UPL = HP / kLPC;           // hidden units per lane: n = sub * UPL + j
  const SmallNetView v = small_net_view(HP, dim);
  const int n0 = sub * UPL;
#pragma unroll
  for (int j = 0; j < UPL; ++j) h1[j] = L[v.b1 + n0 + j] + tc * L[v.wt + n0 + j] + ts * L[v.wt + HP + n0 + j];
#pragma unroll
  for (int k = 0; k < kMaxDim; ++k) {
    if (k < dim) {
#pragma unroll
      for (int j = 0; j < UPL; ++j)
        h1[j] += a[k] * L[v.w1 + k * HP + n0 + j] + b[k] * L[v.w1 + (dim + k) * HP + n0 + j];
    }
  }
  __syncthreads();                          // previous readers of hrow are done
#pragma unroll
  for (int j = 0; j < UPL; ++j) {
    h1[j] = relu_nan(h1[j]);
    hrow[n0 + j] = h1[j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < UPL; ++j) h2[j] = L[v.bh + n0 + j];
  // four input units per step: one 16-byte read of the hidden row (broadcast within the chain's 16 lanes) instead of
  // four scalar ones -- the loop is LDS-issue-bound (one weight read per UPL multiply-adds); same summation order
  using hvec4 = __attribute__((ext_vector_type(4))) float;
#pragma unroll 4
  for (int k = 0; k < HP; k += 4) {
    const hvec4 hv = *reinterpret_cast<const hvec4*>(hrow + k);
    const float* w = L + v.wh + k * HP + n0;
#pragma unroll
    for (int j = 0; j < UPL; ++j) {
      h2[j] += hv[0] * w[j];
      h2[j] += hv[1] * w[HP + j];
      h2[j] += hv[2] * w[2 * HP + j];
      h2[j] += hv[3] * w[3 * HP + j];
    }
  }
#pragma unroll
  for (int j = 0; j < UPL; ++j) h2[j] = relu_nan(h2[j]);
  // heads: k-split over the lanes, 16-lane butterfly
#pragma unroll
  for (int d = 0; d < kMaxDim; ++d) {
    if (d < dim) {
      float ps = 0.f, pt = 0.f, pq = 0.f;
      const float* ws = L + v.whd + (0 * dim + d) * HP + n0;
      const float* wt = L + v.whd + (1 * dim + d) * HP + n0;
      const float* wq = L + v.whd + (2 * dim + d) * HP + n0;
#pragma unroll
      for (int j = 0; j < UPL; ++j) {
        ps += h2[j] * ws[j];
        pt += h2[j] * wt[j];
        pq += h2[j] * wq[j];
      }
      // the chain's sixteen lanes are one DPP row: four VALU steps each instead of four ds_bpermute round trips
      static_assert(kLPC == 16, "row16_sum reduces over the 16 lanes of a chain");
      ps = row16_sum(ps);
      pt = row16_sum(pt);
      pq = row16_sum(pq);
      const float s = ps + L[v.bhd + d], t = pt + L[v.bhd + dim + d], q = pq + L[v.bhd + 2 * dim + d];
      S[d] = tanhf(s) * L[v.es + d];
      T[d] = t;
      Q[d] = (q_tanh ? tanhf(q) : q) * L[v.eq + d];
    }
  }
}

struct TargetView {   // LDS image of l2hmc_mog_target
  int mu, prec, logc, size;
};
__host__ __device__ inline TargetView target_view(int dim, int K) {
  TargetView t;
  t.mu = 0;
  t.prec = K * dim;
  t.logc = t.prec + K * dim * dim;
  t.size = (t.logc + K + 3) & ~3;
  return t;
}

// The target's kind and the scalars of the analytic kinds (wave-uniform: they come from the kernel's arguments).
struct TargetKind {
  int kind;            // L2HMC_TARGET_*
  float eps, a;        // rough well: a = eps * eps, or eps when `easy` (distributions.py:110-116)
};
__host__ __device__ inline TargetKind target_kind(const l2hmc_mog_target& t) {
  TargetKind k;
  k.kind = t.is_gaussian;
  k.eps = k.a = 1.f;
  if (t.is_gaussian == L2HMC_TARGET_ROUGH_WELL) {
    k.eps = t.rough_well.eps;
    k.a = t.rough_well.easy ? k.eps : k.eps * k.eps;
  }
  return k;
}
__host__ __device__ inline bool target_is_analytic(int kind) { return kind >= L2HMC_TARGET_ROUGH_WELL; }

// The funnel's constants (distributions.py:185-188: sigma = 2, clip = 4 sigma whatever the constructor is given)
constexpr float kFunnelInvVar = 0.25f, kFunnelClip = 8.f;
constexpr float kFunnelSMax = 2980.9579870417283f, kFunnelSMin = 3.3546262790251185e-4f;   // exp(+-clip)
constexpr float kLog2Pi = 1.8378770664093453f;

// s = exp(v) of the funnel, or the constant of the clipped branch (tf.where on tf.greater: v == +-clip is unclipped);
// *inv_s = 1 / s, *log_s = log(s), *clipped tells which
__device__ __forceinline__ void funnel_scale(float v, float* inv_s, float* log_s, bool* clipped) {
  const bool hi = v > kFunnelClip, lo = -kFunnelClip > v;
  *clipped = hi || lo;
  *log_s = hi ? kFunnelClip : lo ? -kFunnelClip : v;
  *inv_s = hi ? kFunnelSMin : lo ? kFunnelSMax : expf(-v);
}

// Rough well (distributions.py:101-121) and Gaussian funnel (:184-211), gradient in closed form.  E == nullptr:
// gradient only (the rough well then needs no cosine, the funnel no logarithm term).
template <int MD>
__device__ __forceinline__ void analytic_energy_grad(const TargetKind& tk, int dim, float inv_temp, const float* x,
                                                     float* E, float* g) {
  if (tk.kind == L2HMC_TARGET_ROUGH_WELL) {
    const float c1 = tk.eps / tk.a;
    float n = 0.f, sc = 0.f;
#pragma unroll
    for (int i = 0; i < MD; ++i) {
      g[i] = 0.f;
      if (i < dim) {
        const float t = x[i] / tk.a;
        g[i] = (x[i] - c1 * sinf(t)) * inv_temp;
        if (E) {
          n += x[i] * x[i];
          sc += cosf(t);
        }
      }
    }
    if (E) *E = (0.5f * n + tk.eps * sc) * inv_temp;
  } else {
    float inv_s, log_s, ss = 0.f;
    bool clipped;
    funnel_scale(x[0], &inv_s, &log_s, &clipped);
    const float nn = (float)(dim - 1);
#pragma unroll
    for (int i = 1; i < MD; ++i) {
      g[i] = 0.f;
      if (i < dim) {
        ss += x[i] * x[i];
        g[i] = x[i] * inv_s * inv_temp;
      }
    }
    const float q = ss * inv_s;
    g[0] = (x[0] * kFunnelInvVar + (clipped ? 0.f : 0.5f * (nn - q))) * inv_temp;
    if (E) *E = 0.5f * (x[0] * x[0] * kFunnelInvVar + q + nn * (kLog2Pi + log_s)) * inv_temp;
  }
}

// Hessian(energy)(x) . u of the two analytic kinds: diagonal for the rough well; for the funnel the arrow matrix of
// the selected branch (clipped: diagonal)
template <int MD>
__device__ __forceinline__ void analytic_hvp(const TargetKind& tk, int dim, float inv_temp, const float* x,
                                             const float* u, float* out) {
  if (tk.kind == L2HMC_TARGET_ROUGH_WELL) {
    const float c2 = tk.eps / (tk.a * tk.a);
#pragma unroll
    for (int i = 0; i < MD; ++i) out[i] = i < dim ? (1.f - c2 * cosf(x[i] / tk.a)) * u[i] * inv_temp : 0.f;
  } else {
    float inv_s, log_s, ss = 0.f, xu = 0.f;
    bool clipped;
    funnel_scale(x[0], &inv_s, &log_s, &clipped);
    (void)log_s;
#pragma unroll
    for (int i = 1; i < MD; ++i) {
      out[i] = 0.f;
      if (i < dim) {
        ss += x[i] * x[i];
        xu += x[i] * u[i];
        out[i] = (u[i] - (clipped ? 0.f : x[i] * u[0])) * inv_s * inv_temp;
      }
    }
    const float h00 = kFunnelInvVar + (clipped ? 0.f : 0.5f * ss * inv_s);
    out[0] = (h00 * u[0] - (clipped ? 0.f : xu * inv_s)) * inv_temp;
  }
}

// distributions.py:151-158 (GMM), :63-68 (Gaussian); gradient in closed form.  All loops over the dimension run
// to the compile-time bound MD with a guard, so x / g stay in registers (no dynamically indexed arrays).
// AN: the instance of the analytic kinds (rough well, funnel).  A compile-time flag, not a branch on the kind: sinf /
// cosf carry their large-argument reduction (16 bytes of scratch and about ten registers), which as a run-time branch
// cost four of the mixture's kernel instances a wave per SIMD (profiles/analytic_targets.txt); the AN = false
// instances are the code they were.
template <int MD = L2HMC_MAX_SMALL_DIM, bool AN = false>
__device__ inline void energy_grad(const float* Lt, int dim, int K, const TargetKind& tk, float inv_temp, const float* x,
                                   float* E, float* g) {
  if constexpr (AN) {
    analytic_energy_grad<MD>(tk, dim, inv_temp, x, E, g);
    return;
  }
  const int is_gaussian = tk.kind;
  const TargetView tv = target_view(dim, K);
  float V[kMaxMix];
  float vmax = -INFINITY;
#pragma unroll
  for (int k = 0; k < kMaxMix; ++k) {
    if (k < K) {
      float quad = 0.f;
#pragma unroll
      for (int i = 0; i < MD; ++i) {
        if (i < dim) {
          float pd = 0.f;
#pragma unroll
          for (int j = 0; j < MD; ++j)
            if (j < dim) pd += Lt[tv.prec + (k * dim + i) * dim + j] * (x[j] - Lt[tv.mu + k * dim + j]);
          quad += (x[i] - Lt[tv.mu + k * dim + i]) * pd;
        }
      }
      V[k] = -0.5f * quad + (is_gaussian ? 0.f : Lt[tv.logc + k]);
      vmax = fmaxf(vmax, V[k]);
    }
  }
  float sw = 0.f;
#pragma unroll
  for (int d = 0; d < MD; ++d) g[d] = 0.f;
#pragma unroll
  for (int k = 0; k < kMaxMix; ++k) {
    if (k < K) {
      const float w = is_gaussian ? 1.f : expf(V[k] - vmax);
      sw += w;
#pragma unroll
      for (int i = 0; i < MD; ++i) {
        if (i < dim) {
          float gi = 0.f;
#pragma unroll
          for (int j = 0; j < MD; ++j) {
            if (j < dim) {
              const float dj = x[j] - Lt[tv.mu + k * dim + j];
              gi += (Lt[tv.prec + (k * dim + i) * dim + j] + Lt[tv.prec + (k * dim + j) * dim + i]) * dj;
            }
          }
          g[i] += w * 0.5f * gi;
        }
      }
    }
  }
  const float e = is_gaussian ? -V[0] : -(vmax + logf(sw));
  *E = e * inv_temp;
#pragma unroll
  for (int d = 0; d < MD; ++d) g[d] = g[d] / sw * inv_temp;
}

// (the analytic kinds have no parameter arrays: nothing is staged, and mu / prec / log_const are not pointers to read)
__device__ inline void load_target(const l2hmc_mog_target& t, float* Lt) {
  if (target_is_analytic(t.is_gaussian)) return;
  const TargetView tv = target_view(t.dim, t.K);
  for (int i = threadIdx.x; i < t.K * t.dim; i += blockDim.x) Lt[tv.mu + i] = t.mu[i];
  for (int i = threadIdx.x; i < t.K * t.dim * t.dim; i += blockDim.x) Lt[tv.prec + i] = t.prec[i];
  for (int i = threadIdx.x; i < t.K; i += blockDim.x) Lt[tv.logc + i] = t.is_gaussian ? 0.f : t.log_const[i];
}

// What every entry that takes a target checks before any launch.
inline int check_target_args(const l2hmc_mog_target* t, const char* who) {
  L2HMC_REQUIRE(t != nullptr, "%s: target is NULL", who);
  L2HMC_REQUIRE(t->dim > 0 && t->dim <= kMaxDim && t->K > 0 && t->K <= kMaxMix,
                "%s: target dim=%d (max %d), K=%d (max %d)", who, t->dim, kMaxDim, t->K, kMaxMix);
  const int kind = t->is_gaussian;
  L2HMC_REQUIRE(kind >= L2HMC_TARGET_MIXTURE && kind <= L2HMC_TARGET_FUNNEL,
                "%s: target kind %d unknown (0 mixture, 1 gaussian, 2 rough well, 3 funnel)", who, kind);
  L2HMC_REQUIRE(t->temperature > 0.f, "%s: target temperature must be > 0", who);
  if (kind == L2HMC_TARGET_ROUGH_WELL) {
    L2HMC_REQUIRE(t->K == 1, "%s: rough-well target needs K == 1", who);
    L2HMC_REQUIRE(t->rough_well.eps > 0.f && t->rough_well.eps <= 3.0e38f,
                  "%s: rough-well target needs a finite eps > 0 (eps=%g)", who, (double)t->rough_well.eps);
  } else if (kind == L2HMC_TARGET_FUNNEL) {
    L2HMC_REQUIRE(t->K == 1, "%s: funnel target needs K == 1", who);
    L2HMC_REQUIRE(t->dim >= 2, "%s: funnel target needs dim >= 2 (dim=%d)", who, t->dim);
  } else {
    L2HMC_REQUIRE(t->mu && t->prec && (kind == L2HMC_TARGET_GAUSSIAN || t->log_const), "%s: target has a NULL parameter pointer", who);
    L2HMC_REQUIRE(kind != L2HMC_TARGET_GAUSSIAN || t->K == 1, "%s: gaussian target needs K == 1", who);
  }
  return L2HMC_OK;
}

// What every entry that takes a plan checks before any launch: the target, the plan's dimension against it, the masks;
// need_nets (every plan but a plain-HMC one): a hidden width the kernels have an instance for.
inline int check_small_plan(const l2hmc_small_plan* plan, const char* who, bool need_nets) {
  L2HMC_REQUIRE(plan->x_dim == plan->target.dim, "%s: x_dim=%d != target dim=%d", who, plan->x_dim, plan->target.dim);
  if (int e = check_target_args(&plan->target, who)) return e;
  L2HMC_REQUIRE(plan->trajectory_length > 0 && plan->masks != nullptr, "%s: bad trajectory_length / masks", who);
  L2HMC_REQUIRE(!need_nets || (plan->num_nodes > 0 && plan->num_nodes <= 64), "%s: num_nodes=%d unsupported (1..64)",
                who, plan->num_nodes);
  return L2HMC_OK;
}

// ... and of its two networks: the plan's shape, no NULL weight.  (Apart from check_small_plan: the training entries
// return for an empty batch in between.)
inline int check_small_nets(const l2hmc_small_plan* plan, const char* who) {
  const int dim = plan->x_dim, H = plan->num_nodes;
  const l2hmc_dense_net* nets[2] = {&plan->xnet, &plan->vnet};
  for (const l2hmc_dense_net* n : nets) {
    L2HMC_REQUIRE(n->D == dim && n->Ka == dim && n->Kb == dim && n->H == H,
                  "%s: net shape (D=%d Ka=%d Kb=%d H=%d) != (x_dim=%d, num_nodes=%d)", who, n->D, n->Ka, n->Kb, n->H,
                  dim, H);
    L2HMC_REQUIRE(n->w1_t && n->wt && n->b1 && n->wh_t && n->bh && n->whd_t && n->bhd && n->coeff_s && n->coeff_q,
                  "%s: net has NULL weight pointer", who);
  }
  return L2HMC_OK;
}

// What the run entries (l2hmc_small_run, _run_tempered, _hmc_run) check of their own arguments; a step draws from
// `streams` Philox streams.  (Temperatures and step sizes live on the device and are not looked at.)
inline int check_small_run_args(const char* who, const l2hmc_small_plan* plan, const float* x_in, const float* x_next,
                                int64_t B, uint64_t draw0, int32_t n_steps, int streams, int64_t step_stride,
                                int64_t chain_stride) {
  L2HMC_REQUIRE(plan != nullptr, "%s: plan is NULL", who);
  L2HMC_REQUIRE(x_in != nullptr && x_next != nullptr, "%s: x_in / x_next is NULL", who);
  L2HMC_REQUIRE(B >= 0, "%s: B < 0", who);
  L2HMC_REQUIRE(n_steps > 0, "%s: n_steps=%d must be positive", who, n_steps);
  L2HMC_REQUIRE((uint64_t)streams * (uint64_t)n_steps <= UINT64_MAX - draw0,
                "%s: draw0 + %d * n_steps overflows 64 bits (draw0=%llu, n_steps=%d)", who, streams,
                (unsigned long long)draw0, n_steps);
  L2HMC_REQUIRE(step_stride >= 0 && chain_stride >= 0, "%s: negative stride (step_stride=%lld, chain_stride=%lld)",
                who, (long long)step_stride, (long long)chain_stride);
  return L2HMC_OK;
}

// element i of the stream l2hmc_fill_uniform / l2hmc_fill_normal writes for (seed, offset)   (capi.hip: fill_kernel)
__device__ __forceinline__ void philox_block_at(uint64_t seed, uint64_t offset, int64_t i, uint32_t c[4]) {
  const uint64_t b = (uint64_t)i >> 2;
  c[0] = (uint32_t)b; c[1] = (uint32_t)(b >> 32); c[2] = (uint32_t)offset; c[3] = (uint32_t)(offset >> 32);
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
}
__device__ __forceinline__ float philox_uniform_at(uint64_t seed, uint64_t offset, int64_t i) {
  uint32_t c[4];
  philox_block_at(seed, offset, i, c);
  return (float)(c[i & 3] >> 8) * (1.0f / 16777216.0f);
}
__device__ __forceinline__ float philox_normal_at(uint64_t seed, uint64_t offset, int64_t i) {
  uint32_t c[4];
  philox_block_at(seed, offset, i, c);
  float v[4];
  philox_normal4(c, v);
  return v[i & 3];
}

// Target parameters in registers (x_dim <= 2 instance, the reference's toy targets): energy_grad() re-reads
// them from LDS with run-time offsets at every one of its 2 N + 2 calls, behind the network's LDS traffic; here
// they are read once.  Same arithmetic, same order as energy_grad (small_mlp.h).
template <int MD>
struct TargetRegs {
  static constexpr int KM = 2;              // components held (mog_model.py: two; more fall back to energy_grad)
  static constexpr bool kFits = MD <= 2;
  float mu[KM][MD], prec[KM][MD][MD], logc[KM];
  __device__ __forceinline__ void load(const float* Lt, int dim, int K) {
    const TargetView tv = target_view(dim, K);
#pragma unroll
    for (int k = 0; k < KM; ++k) {
      logc[k] = k < K ? Lt[tv.logc + k] : 0.f;
#pragma unroll
      for (int i = 0; i < MD; ++i) {
        mu[k][i] = (k < K && i < dim) ? Lt[tv.mu + k * dim + i] : 0.f;
#pragma unroll
        for (int j = 0; j < MD; ++j)
          prec[k][i][j] = (k < K && i < dim && j < dim) ? Lt[tv.prec + (k * dim + i) * dim + j] : 0.f;
      }
    }
  }
  // E == nullptr: gradient only (the energy's logf is needed at the two ends of a trajectory, not inside it)
  __device__ __forceinline__ void eval(int dim, int K, int is_gaussian, float inv_temp, const float (&x)[MD], float* E,
                                       float (&g)[MD]) const {
    float V[KM];
    float vmax = -INFINITY;
#pragma unroll
    for (int k = 0; k < KM; ++k) {
      if (k < K) {
        float quad = 0.f;
#pragma unroll
        for (int i = 0; i < MD; ++i) {
          if (i < dim) {
            float pd = 0.f;
#pragma unroll
            for (int j = 0; j < MD; ++j)
              if (j < dim) pd += prec[k][i][j] * (x[j] - mu[k][j]);
            quad += (x[i] - mu[k][i]) * pd;
          }
        }
        V[k] = -0.5f * quad + (is_gaussian ? 0.f : logc[k]);
        vmax = fmaxf(vmax, V[k]);
      }
    }
    float sw = 0.f;
#pragma unroll
    for (int d = 0; d < MD; ++d) g[d] = 0.f;
#pragma unroll
    for (int k = 0; k < KM; ++k) {
      if (k < K) {
        const float w = is_gaussian ? 1.f : expf(V[k] - vmax);
        sw += w;
#pragma unroll
        for (int i = 0; i < MD; ++i) {
          if (i < dim) {
            float gi = 0.f;
#pragma unroll
            for (int j = 0; j < MD; ++j)
              if (j < dim) gi += (prec[k][i][j] + prec[k][j][i]) * (x[j] - mu[k][j]);
            g[i] += w * 0.5f * gi;
          }
        }
      }
    }
    if (E) {
      const float e = is_gaussian ? -V[0] : -(vmax + logf(sw));
      *E = e * inv_temp;
    }
#pragma unroll
    for (int d = 0; d < MD; ++d) g[d] = g[d] / sw * inv_temp;
  }
};

}  // namespace l2hmc
