// One whole MCMC step on device-resident chains (the inference step harness of
// l2hmc/gauge_model.py:1371-1388 around dynamics/gauge_dynamics.py:195-259):
//   draw momenta / direction coin / MH uniform  ->  both trajectories  ->  mix, accept/reject,
//   per-step observables, wrap to [0, 2 pi).  Plans with a whole-trajectory kernel run the step in ONE launch
//   (launch_fused_step, fused_traj.hip: the kernel draws its own Philox streams and finishes the step in its
//   epilogue; launch_hmc_step, hmc_step.hip: the same for plain HMC at any lattice shape); other plans go through the public ops below with the draws of step_draws_kernel.
// The reference pays one session run with a host round trip of the whole batch per step.
#include <vector>

#include "stq_dense.h"

namespace l2hmc {

// elements [0, nV) are standard normals of stream (seed, 2*draw), elements of `cu` uniforms of stream
// (seed, 2*draw+1): bit-identical to l2hmc_fill_normal / l2hmc_fill_uniform with those offsets.
__global__ __launch_bounds__(256) void step_draws_kernel(float* __restrict__ V, int64_t nV, float* __restrict__ cu,
                                                         int64_t ncu, uint64_t seed, uint64_t draw,
                                                         float* __restrict__ sums) {
  const int64_t nbV = (nV + 3) >> 2, nbU = (ncu + 3) >> 2;
  for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nbV + nbU;
       b += (int64_t)gridDim.x * blockDim.x) {
    const bool normal = b < nbV;
    const int64_t blk = normal ? b : b - nbV;
    const uint64_t off = 2 * draw + (normal ? 0 : 1);
    uint32_t c[4] = {(uint32_t)blk, (uint32_t)((uint64_t)blk >> 32), (uint32_t)off, (uint32_t)(off >> 32)};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    float v[4];
    if (normal) {
      philox_normal4(c, v);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = (float)(c[j] >> 8) * (1.0f / 16777216.0f);
    }
    float* out = normal ? V : cu;
    const int64_t n = normal ? nV : ncu, i0 = blk << 2;
    for (int j = 0; j < 4 && i0 + j < n; ++j) out[i0 + j] = v[j];
  }
}

__global__ void charge_diff_kernel(const float* __restrict__ q_in, const float* __restrict__ q_out, int64_t B,
                                   float* __restrict__ charges, float* __restrict__ dq) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  if (charges) charges[i] = q_in[i];
  if (dq) dq[i] = fabsf(q_in[i] - q_out[i]);
}

// general path: [sum p, sum |dQ|, B] from the per-chain arrays, one workgroup, fixed order
__global__ __launch_bounds__(256) void step_sums_kernel(const float* __restrict__ px, const float* __restrict__ dq,
                                                        int64_t B, float* __restrict__ sums) {
  __shared__ float red[2][4];
  float a = 0.f, b = 0.f;
  for (int64_t i = threadIdx.x; i < B; i += 256) {
    a += px[i];
    b += dq[i];
  }
  a = wave_sum(a);
  b = wave_sum(b);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = a;
    red[1][threadIdx.x >> 6] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    sums[0] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    sums[1] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    sums[2] = (float)B;
  }
}

}  // namespace l2hmc

using namespace l2hmc;

static size_t step_head_bytes(int64_t B, int D) {
  return 2 * align_up(sizeof(float) * (size_t)2 * B * D, 256) + align_up(sizeof(float) * (size_t)2 * B, 256) +
         align_up(sizeof(float) * (size_t)2 * B, 256);
}

extern "C" size_t l2hmc_gauge_mcmc_step_ws_bytes(const l2hmc_gauge_plan* plan, int64_t B) {
  if (!plan || B < 0) return 0;
  // the rest behind the head: the general path's transition workspace and outputs, or the one-launch step's hand-off
  const size_t general = l2hmc_gauge_transition_ws_bytes(plan, B, 1) +
                         3 * align_up(sizeof(float) * (size_t)B * 2 * plan->T * plan->X, 256);
  const size_t hand = fused_step_hand_bytes(B, 2 * plan->T * plan->X);
  return step_head_bytes(B, 2 * plan->T * plan->X) + (general > hand ? general : hand);
}

extern "C" int l2hmc_gauge_mcmc_step(const l2hmc_gauge_plan* plan, float beta, float* x, int64_t B, uint64_t seed,
                                     uint64_t draw, float* px, float* actions, float* plaqs, float* charges,
                                     float* charge_diff, void* ws, size_t ws_bytes, l2hmc_stream_t stream) {
  return l2hmc_gauge_mcmc_step_ex(plan, beta, x, x, B, seed, draw, px, actions, plaqs, charges, charge_diff, nullptr,
                                  ws, ws_bytes, stream);
}

// The step of l2hmc_gauge_mcmc_step_ex (`who` = its name in messages) on checked pointers and B > 0.  betas: NULL, or
// the ladder of l2hmc_gauge_mcmc_step_ladder (DEVICE; chain c at betas[c * chain_stride]; `beta` is then not read by a
// live chain).
static int mcmc_step_impl(const char* who, const l2hmc_gauge_plan* plan, float beta, const float* betas,
                          int64_t chain_stride, const float* x_in, float* x_next, int64_t B, uint64_t seed,
                          uint64_t draw, float* px, float* actions, float* plaqs, float* charges, float* charge_diff,
                          float* step_sums, void* ws, size_t ws_bytes, l2hmc_stream_t stream) {
  const float* x = x_in;
  const size_t need = l2hmc_gauge_mcmc_step_ws_bytes(plan, B);
  if (ws_bytes < need) {
    set_error("%s: workspace %zu < %zu bytes", who, ws_bytes, need);
    return L2HMC_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  const int T = plan->T, X = plan->X, D = 2 * T * X;
  char* base = static_cast<char*>(ws);
  const size_t xv = align_up(sizeof(float) * (size_t)2 * B * D, 256);
  float* Xw = reinterpret_cast<float*>(base);
  float* Vw = reinterpret_cast<float*>(base + xv);
  float* Pw = reinterpret_cast<float*>(base + 2 * xv);
  float* cu = reinterpret_cast<float*>(base + 2 * xv + align_up(sizeof(float) * (size_t)2 * B, 256));
  char* rest = base + step_head_bytes(B, D);
  size_t rest_bytes = ws_bytes - step_head_bytes(B, D);

  const bool fused = !(plan->flags & L2HMC_PLAN_LAYERED) && fused_plan_supported(plan);
  const bool selected = (plan->flags & L2HMC_PLAN_SELECTED_ONLY) != 0;
  if (!(plan->flags & L2HMC_PLAN_LAYERED) && hmc_plan_supported(plan))
    // plain HMC: ONE launch as well (hmc_step.hip), at any lattice of up to 1024 sites
    return launch_hmc_step(plan, beta, x, x_next, B, seed, draw, selected ? 0 : 1, px, actions, plaqs, charges,
                           charge_diff, step_sums, Xw /* 2 floats per workgroup of scratch */, s);
  if (fused) {
    // ONE launch: the whole-trajectory kernel draws, integrates, mixes, accepts, measures and wraps (fused_traj.hip)
    return launch_fused_step(plan, beta, x, x_next, B, seed, draw, selected ? 0 : 1, px, actions, plaqs, charges,
                             charge_diff, step_sums, Xw /* 2 * workgroups floats of scratch */, rest, s, nullptr, nullptr,
                             nullptr, betas, chain_stride);
  }
  // the layer-by-layer path: the plan's checks (the transition's own) come ahead of its first launch, the draws
  if (int e = gauge_check_plan(plan)) return e;
  // momenta of both directions, coin | u  (tf.random_normal :269, tf.random_uniform :223,:246)
  const int64_t nblk = (((int64_t)2 * B * D + 3) >> 2) + ((2 * B + 3) >> 2);
  hipLaunchKernelGGL(step_draws_kernel, dim3((unsigned)hmin(ceil_div(nblk, 256), 4096)), dim3(256), 0, s, Vw,
                     (int64_t)2 * B * D, cu, 2 * B, seed, draw, nullptr);
  L2HMC_CHECK_LAUNCH("step_draws");

  // general path (no fused kernel for this plan, or an odd lattice): the same step through the public ops
  const size_t bd = align_up(sizeof(float) * (size_t)B * D, 256);
  float* x_prop = reinterpret_cast<float*>(rest);
  float* v_prop = reinterpret_cast<float*>(rest + bd);
  float* x_out = reinterpret_cast<float*>(rest + 2 * bd);
  rest += 3 * bd;
  rest_bytes -= 3 * bd;
  L2HMC_REQUIRE(!step_sums || (px && charge_diff), "%s: step_sums needs px and charge_diff on this path", who);
  float* pp = px ? px : Xw;        // Xw / Pw of the head are free here: the transition carves its own copies
  // (a ladder: rows B + c and c of the stacked [forward; backward] trajectories are chain c)
  const RowBeta rbeta = betas ? RowBeta(betas, B, chain_stride) : RowBeta(beta);
  if (int e = gauge_transition_rows(who, plan, rbeta, x, Vw, Vw + (size_t)B * D, cu, cu + B, B, selected ? 0 : 1, x_prop,
                                    v_prop, pp, x_out, rest, rest_bytes, s))
    return e;
  float* q_in = Pw;
  float* q_out = Pw + B;
  if (int e = l2hmc_u1_action_force(x, B, T, X, beta, actions, nullptr, plaqs, q_in, stream)) return e;
  if (int e = l2hmc_u1_action_force(x_out, B, T, X, beta, nullptr, nullptr, nullptr, q_out, stream)) return e;
  hipLaunchKernelGGL(charge_diff_kernel, dim3((unsigned)ceil_div(B, 256)), dim3(256), 0, s, q_in, q_out, B, charges,
                     charge_diff);
  L2HMC_CHECK_LAUNCH("charge_diff");
  if (step_sums) {
    hipLaunchKernelGGL(step_sums_kernel, dim3(1), dim3(256), 0, s, px, charge_diff, B, step_sums);
    L2HMC_CHECK_LAUNCH("step_sums");
  }
  return l2hmc_wrap_angle(x_out, (int64_t)B * D, x_next, stream);
}

extern "C" int l2hmc_gauge_mcmc_step_ex(const l2hmc_gauge_plan* plan, float beta, const float* x_in, float* x_next,
                                        int64_t B, uint64_t seed, uint64_t draw, float* px, float* actions,
                                        float* plaqs, float* charges, float* charge_diff, float* step_sums, void* ws,
                                        size_t ws_bytes, l2hmc_stream_t stream) {
  L2HMC_REQUIRE(plan != nullptr && B >= 0, "gauge_mcmc_step: bad arguments");
  // the step takes the streams 2 * draw and 2 * draw + 1: from 2^63 on they would wrap onto those of draw - 2^63
  L2HMC_REQUIRE(draw < (1ull << 63), "gauge_mcmc_step: draw = %llu is not below 2^63", (unsigned long long)draw);
  if (B == 0) return L2HMC_OK;
  L2HMC_REQUIRE(x_in && x_next && ws, "gauge_mcmc_step: NULL pointer");
  return mcmc_step_impl("gauge_mcmc_step", plan, beta, nullptr, 0, x_in, x_next, B, seed, draw, px, actions, plaqs,
                        charges, charge_diff, step_sums, ws, ws_bytes, stream);
}

// ---- the same step with a beta per chain: the whole-step kernels' LADDER instances, or the layer-by-layer path with
// the rows' betas (RowBeta) -- every L2HMC plan
extern "C" int l2hmc_gauge_mcmc_step_ladder(const l2hmc_gauge_plan* plan, const float* betas, int64_t chain_stride,
                                            const float* x_in, float* x_next, int64_t B, uint64_t seed, uint64_t draw,
                                            float* px, float* actions, float* plaqs, float* charges,
                                            float* charge_diff, float* step_sums, void* ws, size_t ws_bytes,
                                            l2hmc_stream_t stream) {
  const char* who = "gauge_mcmc_step_ladder";
  L2HMC_REQUIRE(plan != nullptr, "%s: plan is NULL", who);
  L2HMC_REQUIRE(!plan->hmc, "%s: plan.hmc = 1: l2hmc_gauge_hmc_run_ladder runs plain HMC with a beta per chain", who);
  L2HMC_REQUIRE(betas != nullptr, "%s: NULL betas", who);
  L2HMC_REQUIRE(chain_stride == 0 || chain_stride == 1, "%s: chain_stride = %lld is not 0 or 1", who,
                (long long)chain_stride);
  L2HMC_REQUIRE(x_in && x_next, "%s: NULL x_in / x_next", who);
  L2HMC_REQUIRE(B >= 0, "%s: B < 0", who);
  L2HMC_REQUIRE(draw < (1ull << 63), "%s: draw = %llu is not below 2^63", who, (unsigned long long)draw);
  if (B == 0) return L2HMC_OK;
  if (!ws) ws_bytes = 0;
  return mcmc_step_impl(who, plan, 0.f, betas, chain_stride, x_in, x_next, B, seed, draw, px, actions, plaqs, charges,
                        charge_diff, step_sums, ws, ws_bytes, stream);
}

extern "C" int l2hmc_gauge_transition_draw(const l2hmc_gauge_plan* plan, float beta, const float* x, int64_t B,
                                           uint64_t seed, uint64_t draw, float* x_prop, float* v_prop,
                                           float* p_accept, float* x_out, void* ws, size_t ws_bytes,
                                           l2hmc_stream_t stream) {
  L2HMC_REQUIRE(plan != nullptr && B >= 0, "gauge_transition_draw: bad arguments");
  L2HMC_REQUIRE(draw < (1ull << 63), "gauge_transition_draw: draw = %llu is not below 2^63", (unsigned long long)draw);
  if (B == 0) return L2HMC_OK;
  L2HMC_REQUIRE(x && x_prop && v_prop && p_accept && x_out && ws, "gauge_transition_draw: NULL pointer");
  const size_t need = l2hmc_gauge_mcmc_step_ws_bytes(plan, B);
  if (ws_bytes < need) {
    set_error("gauge_transition_draw: workspace %zu < %zu bytes", ws_bytes, need);
    return L2HMC_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  const int D = 2 * plan->T * plan->X;
  const bool selected = (plan->flags & L2HMC_PLAN_SELECTED_ONLY) != 0;
  if (!(plan->flags & L2HMC_PLAN_LAYERED) && hmc_plan_supported(plan))
    return launch_hmc_step(plan, beta, x, nullptr, B, seed, draw, selected ? 0 : 1, p_accept, nullptr, nullptr, nullptr,
                           nullptr, nullptr, nullptr, s, x_prop, v_prop, x_out);
  if (!(plan->flags & L2HMC_PLAN_LAYERED) && fused_plan_supported(plan))
    return launch_fused_step(plan, beta, x, nullptr, B, seed, draw, selected ? 0 : 1, p_accept, nullptr, nullptr,
                             nullptr, nullptr, nullptr, nullptr, static_cast<char*>(ws) + step_head_bytes(B, D), s,
                             x_prop, v_prop, x_out);
  // other plans: the same draws into the workspace, then the public transition
  char* base = static_cast<char*>(ws);
  const size_t xv = align_up(sizeof(float) * (size_t)2 * B * D, 256);
  float* Vw = reinterpret_cast<float*>(base + xv);
  float* cu = reinterpret_cast<float*>(base + 2 * xv + align_up(sizeof(float) * (size_t)2 * B, 256));
  const int64_t nblk = (((int64_t)2 * B * D + 3) >> 2) + ((2 * B + 3) >> 2);
  hipLaunchKernelGGL(step_draws_kernel, dim3((unsigned)hmin(ceil_div(nblk, 256), 4096)), dim3(256), 0, s, Vw,
                     (int64_t)2 * B * D, cu, 2 * B, seed, draw, nullptr);
  L2HMC_CHECK_LAUNCH("step_draws");
  char* rest = base + step_head_bytes(B, D);
  return l2hmc_gauge_transition(plan, beta, x, Vw, Vw + (size_t)B * D, cu, cu + B, B, selected ? 0 : 1, x_prop, v_prop,
                                p_accept, x_out, rest, ws_bytes - step_head_bytes(B, D), stream);
}

// ---- a run of plain-HMC steps: one launch where the plan has the one-launch kernel, the loop over the step otherwise
static bool hmc_run_one_launch(const l2hmc_gauge_plan* plan) {
  return !(plan->flags & L2HMC_PLAN_LAYERED) && hmc_plan_supported(plan);
}

static size_t hmc_run_loop_scratch(int64_t B) { return align_up(sizeof(float) * (size_t)B, 256); }

extern "C" size_t l2hmc_gauge_hmc_run_ws_bytes(const l2hmc_gauge_plan* plan, int64_t B, int32_t n_steps) {
  if (!plan || B < 0 || n_steps <= 0) return 0;
  if (!plan->hmc) {
    set_error("gauge_hmc_run_ws_bytes: plan.hmc = 0 (a run is steps of plain HMC)");
    return 0;
  }
  if (hmc_run_one_launch(plan)) return (size_t)n_steps * hmc_run_part_bytes(B > 0 ? B : 1);
  // the loop: one step's workspace, and px / charge_diff rows for a caller that keeps no histories but wants sums
  return l2hmc_gauge_mcmc_step_ws_bytes(plan, B) + 2 * hmc_run_loop_scratch(B);
}

extern "C" int l2hmc_gauge_hmc_run(const l2hmc_gauge_plan* plan, const float* betas, const float* x_in, float* x_next,
                                   int64_t B, uint64_t seed, uint64_t draw0, int32_t n_steps, float* px,
                                   float* actions, float* plaqs, float* charges, float* charge_diff, float* step_sums,
                                   float* samples, void* ws, size_t ws_bytes, l2hmc_stream_t stream) {
  L2HMC_REQUIRE(plan != nullptr && B >= 0, "gauge_hmc_run: bad arguments");
  L2HMC_REQUIRE(plan->hmc, "gauge_hmc_run: plan.hmc = 0 (a run is steps of plain HMC)");
  L2HMC_REQUIRE(n_steps > 0, "gauge_hmc_run: n_steps = %d, expected at least 1", (int)n_steps);
  L2HMC_REQUIRE(betas != nullptr, "gauge_hmc_run: NULL betas");
  // the run kernel relies on bit 63 of every draw index being 0 (hmc_step.hip: HmcRunArgs)
  L2HMC_REQUIRE(draw0 <= (1ull << 63) - (uint64_t)n_steps, "gauge_hmc_run: draw0 + n_steps exceeds 2^63");
  L2HMC_REQUIRE(x_in && x_next, "gauge_hmc_run: NULL x_in / x_next");
  L2HMC_REQUIRE(!step_sums || ws, "gauge_hmc_run: step_sums needs the workspace");
  if (B == 0) return L2HMC_OK;
  const size_t need = l2hmc_gauge_hmc_run_ws_bytes(plan, B, n_steps);
  if ((step_sums || !hmc_run_one_launch(plan)) && (!ws || ws_bytes < need)) {
    set_error("gauge_hmc_run: workspace %zu < %zu bytes", ws ? ws_bytes : (size_t)0, need);
    return L2HMC_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  const bool selected = (plan->flags & L2HMC_PLAN_SELECTED_ONLY) != 0;
  if (hmc_run_one_launch(plan))
    return launch_hmc_run(plan, betas, x_in, x_next, B, seed, draw0, n_steps, selected ? 0 : 1, px, actions, plaqs,
                          charges, charge_diff, step_sums, samples, step_sums ? static_cast<float*>(ws) : nullptr, s);
  // no one-launch kernel (more than 1024 sites, or L2HMC_PLAN_LAYERED): the same run, step by step.  The loop needs
  // the betas on the host, so it waits for the stream once.
  std::vector<float> hb((size_t)n_steps);
  if (hipMemcpyAsync(hb.data(), betas, sizeof(float) * (size_t)n_steps, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess) {
    set_error("gauge_hmc_run: reading betas: %s", hipGetErrorString(hipGetLastError()));
    return L2HMC_ERR_HIP;
  }
  const size_t D = 2 * (size_t)plan->T * plan->X, sc = hmc_run_loop_scratch(B);
  char* base = static_cast<char*>(ws);
  float* px_s = reinterpret_cast<float*>(base);
  float* dq_s = reinterpret_cast<float*>(base + sc);
  const float* xi = x_in;
  for (int32_t i = 0; i < n_steps; ++i) {
    const size_t row = (size_t)i * (size_t)B;
    float* xo = samples ? samples + row * D : x_next;
    float* sums = step_sums ? step_sums + 4 * (size_t)i : nullptr;
    if (int e = l2hmc_gauge_mcmc_step_ex(plan, hb[i], xi, xo, B, seed, draw0 + (uint64_t)i, px ? px + row : (sums ? px_s : nullptr),
                                         actions ? actions + row : nullptr, plaqs ? plaqs + row : nullptr,
                                         charges ? charges + row : nullptr,
                                         charge_diff ? charge_diff + row : (sums ? dq_s : nullptr), sums, base + 2 * sc,
                                         ws_bytes - 2 * sc, stream))
      return e;
    xi = xo;
  }
  if (samples && hipMemcpyAsync(x_next, xi, sizeof(float) * (size_t)B * D, hipMemcpyDeviceToDevice, s) != hipSuccess) {
    set_error("gauge_hmc_run: copying the final state: %s", hipGetErrorString(hipGetLastError()));
    return L2HMC_ERR_HIP;
  }
  return L2HMC_OK;
}

// ---- the same run with beta per step and chain and a step size per chain (hmc_run_kernel<SPT, true>).  Only plans
// with the one-launch kernel: a ladder is there to fill ONE launch, so there is no host loop to fall back on.
// Returns L2HMC_OK or sets the error; `who` words it for the entry and for its workspace query.
static int hmc_run_ladder_check(const char* who, const l2hmc_gauge_plan* plan, int64_t B, int32_t n_steps) {
  L2HMC_REQUIRE(plan != nullptr, "%s: plan is NULL", who);
  L2HMC_REQUIRE(plan->hmc, "%s: plan.hmc = 0 (a run is steps of plain HMC)", who);
  L2HMC_REQUIRE(hmc_run_one_launch(plan),
                "%s: the plan has no one-launch kernel (more than 1024 sites, or L2HMC_PLAN_LAYERED): "
                "l2hmc_gauge_hmc_run runs it step by step, one beta at a time", who);
  L2HMC_REQUIRE(n_steps > 0, "%s: n_steps = %d, expected at least 1", who, (int)n_steps);
  L2HMC_REQUIRE(B >= 0, "%s: B < 0", who);
  return L2HMC_OK;
}

extern "C" size_t l2hmc_gauge_hmc_run_ladder_ws_bytes(const l2hmc_gauge_plan* plan, int64_t B, int32_t n_steps) {
  if (hmc_run_ladder_check("gauge_hmc_run_ladder_ws_bytes", plan, B, n_steps)) return 0;
  return (size_t)n_steps * hmc_run_part_bytes(B > 0 ? B : 1);
}

extern "C" int l2hmc_gauge_hmc_run_ladder(const l2hmc_gauge_plan* plan, const float* betas, int64_t step_stride,
                                          int64_t chain_stride, const float* eps_chain, const float* x_in,
                                          float* x_next, int64_t B, uint64_t seed, uint64_t draw0, int32_t n_steps,
                                          float* px, float* actions, float* plaqs, float* charges, float* charge_diff,
                                          float* step_sums, float* samples, void* ws, size_t ws_bytes,
                                          l2hmc_stream_t stream) {
  if (int e = hmc_run_ladder_check("gauge_hmc_run_ladder", plan, B, n_steps)) return e;
  L2HMC_REQUIRE(betas != nullptr, "gauge_hmc_run_ladder: NULL betas");
  L2HMC_REQUIRE(step_stride >= 0 && chain_stride >= 0,
                "gauge_hmc_run_ladder: negative stride (step_stride=%lld, chain_stride=%lld)", (long long)step_stride,
                (long long)chain_stride);
  // the run kernel relies on bit 63 of every draw index being 0 (hmc_step.hip: HmcRunArgs)
  L2HMC_REQUIRE(draw0 <= (1ull << 63) - (uint64_t)n_steps, "gauge_hmc_run_ladder: draw0 + n_steps exceeds 2^63");
  L2HMC_REQUIRE(x_in && x_next, "gauge_hmc_run_ladder: NULL x_in / x_next");
  L2HMC_REQUIRE(!step_sums || ws, "gauge_hmc_run_ladder: step_sums needs the workspace");
  if (B == 0) return L2HMC_OK;
  const size_t need = l2hmc_gauge_hmc_run_ladder_ws_bytes(plan, B, n_steps);
  if (step_sums && ws_bytes < need) {
    set_error("gauge_hmc_run_ladder: workspace %zu < %zu bytes", ws_bytes, need);
    return L2HMC_ERR_WORKSPACE;
  }
  const bool selected = (plan->flags & L2HMC_PLAN_SELECTED_ONLY) != 0;
  return launch_hmc_run_ladder(plan, betas, step_stride, chain_stride, eps_chain, x_in, x_next, B, seed, draw0, n_steps,
                               selected ? 0 : 1, px, actions, plaqs, charges, charge_diff, step_sums, samples,
                               step_sums ? static_cast<float*>(ws) : nullptr, (hipStream_t)stream);
}

// ---- the ladder run with the replica-exchange rounds inside the launch (hmc_run_exchange_kernel, hmc_step.hip)
extern "C" int l2hmc_gauge_hmc_run_exchange_served(const l2hmc_gauge_plan* plan, int32_t group) {
  if (!plan) {
    set_error("gauge_hmc_run_exchange_served: plan is NULL");
    return 0;
  }
  char why[384];
  if (hmc_exchange_served(plan, group, why, sizeof(why))) return 1;
  set_error("gauge_hmc_run_exchange_served: not served: %s (l2hmc_gauge_replica_swap between launches of "
            "l2hmc_gauge_hmc_run_ladder takes it)", why);
  return 0;
}

extern "C" size_t l2hmc_gauge_hmc_run_exchange_ws_bytes(const l2hmc_gauge_plan* plan, int64_t B, int32_t n_steps) {
  if (hmc_run_ladder_check("gauge_hmc_run_exchange_ws_bytes", plan, B, n_steps)) return 0;
  return (size_t)n_steps * hmc_run_part_bytes(B > 0 ? B : 1);
}

extern "C" int l2hmc_gauge_hmc_run_exchange(const l2hmc_gauge_plan* plan, const float* betas, int64_t step_stride,
                                            int64_t chain_stride, const float* eps_chain, const float* x_in,
                                            float* x_next, int64_t B, uint64_t seed, uint64_t draw0, int32_t n_steps,
                                            int32_t group, int32_t swap_every, int32_t swap_phase,
                                            int32_t first_parity, int32_t* replica, float* px, float* actions,
                                            float* plaqs, float* charges, float* charge_diff, float* step_sums,
                                            float* samples, float* swap_p, uint8_t* swapped, int32_t* replica_hist,
                                            void* ws, size_t ws_bytes, l2hmc_stream_t stream) {
  const char* who = "gauge_hmc_run_exchange";
  if (int e = hmc_run_ladder_check(who, plan, B, n_steps)) return e;
  L2HMC_REQUIRE(betas != nullptr, "%s: NULL betas (a replica group is a ladder of betas)", who);
  L2HMC_REQUIRE(step_stride >= 0 && chain_stride >= 0, "%s: negative stride (step_stride=%lld, chain_stride=%lld)", who,
                (long long)step_stride, (long long)chain_stride);
  L2HMC_REQUIRE(group >= 2, "%s: group = %d: a replica group has 2 rungs or more", who, group);
  L2HMC_REQUIRE(B % group == 0, "%s: B = %lld is not a multiple of group = %d", who, (long long)B, group);
  L2HMC_REQUIRE(swap_every >= 1, "%s: swap_every = %d must be 1 or more", who, swap_every);
  L2HMC_REQUIRE(swap_phase >= 0 && swap_phase < swap_every, "%s: swap_phase = %d is not in [0, swap_every = %d)", who,
                swap_phase, swap_every);
  L2HMC_REQUIRE(first_parity == 0 || first_parity == 1, "%s: first_parity = %d is not 0 or 1", who, first_parity);
  char why[384];
  L2HMC_REQUIRE(hmc_exchange_served(plan, group, why, sizeof(why)),
                "%s: not served: %s (l2hmc_gauge_replica_swap between launches of l2hmc_gauge_hmc_run_ladder takes it)",
                who, why);
  // a round after step s iff (swap_phase + s + 1) % swap_every == 0; a step or a round moves the draw index by one,
  // and the run kernel relies on bit 63 of every draw index being 0 (hmc_step.hip: HmcRunArgs)
  const uint64_t rounds = ((uint64_t)swap_phase + (uint64_t)n_steps) / (uint64_t)swap_every;
  L2HMC_REQUIRE(draw0 <= (1ull << 63) - (uint64_t)n_steps - rounds,
                "%s: draw0 + n_steps + rounds exceeds 2^63 (draw0=%llu, n_steps=%d, rounds=%llu)", who,
                (unsigned long long)draw0, n_steps, (unsigned long long)rounds);
  L2HMC_REQUIRE(x_in && x_next, "%s: NULL x_in / x_next", who);
  L2HMC_REQUIRE(!step_sums || ws, "%s: step_sums needs the workspace", who);
  if (B == 0) return L2HMC_OK;
  const size_t need = l2hmc_gauge_hmc_run_exchange_ws_bytes(plan, B, n_steps);
  if (step_sums && ws_bytes < need) {
    set_error("%s: workspace %zu < %zu bytes", who, ws_bytes, need);
    return L2HMC_ERR_WORKSPACE;
  }
  const bool selected = (plan->flags & L2HMC_PLAN_SELECTED_ONLY) != 0;
  return launch_hmc_run_exchange(plan, betas, step_stride, chain_stride, eps_chain, x_in, x_next, B, seed, draw0,
                                 n_steps, selected ? 0 : 1, group, swap_every, swap_phase, first_parity, replica, px,
                                 actions, plaqs, charges, charge_diff, step_sums, samples, swap_p, swapped,
                                 replica_hist, step_sums ? static_cast<float*>(ws) : nullptr, (hipStream_t)stream);
}
