// Training path of the layer-by-layer generic Dynamics (any x_dim, num_nodes, energy): the pieces a reverse pass
// over a taped layered trajectory needs -- what tf.gradients(loss, dynamics.variables) builds in
//   l2hmc/mog_model.py:324-363        (loss, optimiser)
// for the graph of
//   l2hmc/utils/dynamics.py:120-225   (sub-updates) and l2hmc/utils/network.py:89-114 (S/T/Q network).
// The orchestration (which sub-update, which tape slice) lives in l2hmc_amd/layered_train.py; every entry here takes
// any positive D, H, Ka, Kb and any row count:
//   * l2hmc_stq_dense_taped: l2hmc_stq_dense with h1 / h2 in caller buffers (same launches, same bits);
//   * l2hmc_lf_update_{v,x}_vjp: reverse of one sub-update (lf_update.h, dense rows);
//   * l2hmc_dense_backward_data: cotangents of (S, T, Q) -> head pre-activations -> h2 -> h1 -> network inputs, on
//     the matrix pipe (gemm_relu_kernel KIND 3 / 4, bounds-checked when widths are ragged);
//   * l2hmc_dense_weight_grads: once per network and step, over all calls' tapes stacked along rows: split-k "TN"
//     MFMA products with bounds-checked staging and column sums, each reduced in a fixed order (no float atomics).
#include "stq_dense.h"
#include "lf_update.h"

namespace l2hmc {

using f32x16_lt = __attribute__((ext_vector_type(16))) float;

// ---------------------------------------------------------------------------------------------------------------
// reverse of lf_update_v_kernel (leapfrog.hip) for ANY cotangents, lf_kick_vjp of lf_update.h: one wave per row.
// Inputs: u = d/dv', dl = d/dlogdet (logdet += sum_d s).  Outputs: dv, dg, dS, dT, dQ [rows][D], deps [rows].
__global__ __launch_bounds__(256) void lf_update_v_vjp_kernel(
    const float* __restrict__ v, const float* __restrict__ g, const float* __restrict__ S, const float* __restrict__ T,
    const float* __restrict__ Q, float eps, int d, int64_t rows, int D, const float* __restrict__ dvo,
    const float* __restrict__ dld, float* __restrict__ dv, float* __restrict__ dg, float* __restrict__ dS,
    float* __restrict__ dT, float* __restrict__ dQ, float* __restrict__ deps) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float dl = dld ? dld[row] : 0.f;
  float de = 0.f;
  for (int c = lane; c < D; c += kWave) {
    const int64_t i = row * D + c;
    lf_kick_vjp(v[i], g[i], S[i], T[i], Q[i], eps, d, dvo[i], dl, dv[i], dg[i], dS[i], dT[i], dQ[i], de);
  }
  de = wave_sum(de);
  if (lane == 0) deps[row] = de;
}

// reverse of lf_update_x_kernel (lf_drift_vjp of lf_update.h; logdet += sum_d (1 - k) s).
// Outputs: dx, dv (the cotangent of v through this update alone), dS, dT, dQ [rows][D], deps [rows].
__global__ __launch_bounds__(256) void lf_update_x_vjp_kernel(
    const float* __restrict__ x, const float* __restrict__ v, const float* __restrict__ keep,
    const float* __restrict__ S, const float* __restrict__ T, const float* __restrict__ Q, float eps, int d,
    int64_t rows, int D, const float* __restrict__ dxo, const float* __restrict__ dld, float* __restrict__ dx,
    float* __restrict__ dv, float* __restrict__ dS, float* __restrict__ dT, float* __restrict__ dQ,
    float* __restrict__ deps) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float dl = dld ? dld[row] : 0.f;
  float de = 0.f;
  for (int c = lane; c < D; c += kWave) {
    const int64_t i = row * D + c;
    float dt, eq;
    lf_drift_vjp(x[i], v[i], keep[c], S[i], T[i], Q[i], eps, d, dxo[i], dl, dx[i], dS[i], dt, dQ[i], eq, de);
    dT[i] = dt;
    dv[i] = dt * eq;
  }
  de = wave_sum(de);
  if (lane == 0) deps[row] = de;
}

// reverse of lf_update_x_ncp_kernel (lf_drift_ncp_vjp of lf_update.h): lf_update_x_vjp_kernel's outputs
__global__ __launch_bounds__(256) void lf_update_x_ncp_vjp_kernel(
    const float* __restrict__ x, const float* __restrict__ v, const float* __restrict__ keep,
    const float* __restrict__ S, const float* __restrict__ T, const float* __restrict__ Q, float eps, int d,
    int64_t rows, int D, const float* __restrict__ dxo, const float* __restrict__ dld, float* __restrict__ dx,
    float* __restrict__ dv, float* __restrict__ dS, float* __restrict__ dT, float* __restrict__ dQ,
    float* __restrict__ deps) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float dl = dld ? dld[row] : 0.f;
  float de = 0.f;
  for (int c = lane; c < D; c += kWave) {
    const int64_t i = row * D + c;
    float dt, eq;
    lf_drift_ncp_vjp(x[i], v[i], keep[c], S[i], T[i], Q[i], eps, d, dxo[i], dl, dx[i], dS[i], dt, dQ[i], eq, de);
    dT[i] = dt;
    dv[i] = dt * eq;
  }
  de = wave_sum(de);
  if (lane == 0) deps[row] = de;
}

// ---------------------------------------------------------------------------------------------------------------
// heads: S = e^{cs} tanh(zS), T = zT, Q = e^{cq} tanh(zQ) (q_tanh) or e^{cq} zQ.  Cotangents of (S, T, Q) ->
// dpre = [dzS | dzT | dzQ] per row, and (optional) dsq = [dS S | dQ Q] per row: d/dcs and d/dcq before the sum over
// rows (dS/dcs = S, dQ/dcq = Q).
__global__ __launch_bounds__(256) void heads_pre_bwd_kernel(
    const float* __restrict__ S, const float* __restrict__ Q, const float* __restrict__ dS, const float* __restrict__ dT,
    const float* __restrict__ dQ, const float* __restrict__ cs, const float* __restrict__ cq, int q_tanh, int64_t rows,
    int D, float* __restrict__ dpre, float* __restrict__ dsq) {
  const int64_t n = rows * D;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / D;
    const int c = (int)(i - row * D);
    const float ecs = expf(cs[c]), ecq = expf(cq[c]);
    const float s = S[i], q = Q[i], ds = dS[i], dq = dQ[i];
    const float th = s / ecs;
    float daq = dq * ecq;
    if (q_tanh) {
      const float tq = q / ecq;
      daq *= 1.f - tq * tq;
    }
    float* o = dpre + row * 3 * D + c;
    o[0] = ds * ecs * (1.f - th * th);
    o[D] = dT[i];
    o[2 * D] = daq;
    if (dsq) {
      dsq[row * 2 * D + c] = ds * s;
      dsq[row * 2 * D + D + c] = dq * q;
    }
  }
}

// out[c][r] = in[r][c]
__global__ __launch_bounds__(256) void lt_transpose_kernel(const float* __restrict__ in, int R, int Cn,
                                                           float* __restrict__ out) {
  __shared__ float t[32][33];
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int k = ty; k < 32; k += 8)
    if (r0 + k < R && c0 + tx < Cn) t[k][tx] = in[(size_t)(r0 + k) * Cn + c0 + tx];
  __syncthreads();
  for (int k = ty; k < 32; k += 8)
    if (c0 + k < Cn && r0 + tx < R) out[(size_t)(c0 + k) * R + r0 + tx] = t[tx][k];
}

// ---------------------------------------------------------------------------------------------------------------
// weight gradients, any widths: part[split][m][n] = sum_{r in split} P[r][m] Q[r][n].  64 x 64 tile per workgroup,
// four waves of one 32x32 fp32 MFMA accumulator (32x32x2) each; 16 contraction rows per stage, staged element-wise
// with bounds checks (rows and columns past the end read 0), so neither the widths nor the row strides need any
// alignment.  The contraction is split over workgroups; the partials are summed in a fixed order afterwards.
constexpr int kTnBM = 64, kTnBN = 64, kTnKR = 16, kTnLD = 64 + 4;
struct TnRaggedArgs {
  const float* P; int ldp; int M;
  const float* Q; int ldq; int N;
  int64_t R, chunk;
  float* part;
  int mt, nt;
};

__global__ __launch_bounds__(256) void tn_ragged_kernel(TnRaggedArgs p) {
  __shared__ float Ps[kTnKR][kTnLD];
  __shared__ float Qs[kTnKR][kTnLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, half = lane >> 5, r = lane & 31;
  const int tiles = p.mt * p.nt;
  const int split = blockIdx.x / tiles, tile = blockIdx.x - split * tiles;
  const int m0 = (tile / p.nt) * kTnBM, n0 = (tile % p.nt) * kTnBN;
  const int64_t rbeg = (int64_t)split * p.chunk;
  const int64_t rend = rbeg + p.chunk < p.R ? rbeg + p.chunk : p.R;
  f32x16_lt acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  for (int64_t rr = rbeg; rr < rend; rr += kTnKR) {
#pragma unroll
    for (int j = 0; j < (kTnKR * kTnBM) / 256; ++j) {
      const int idx = tid + 256 * j;
      const int kr = idx / kTnBM, c = idx - kr * kTnBM;
      const int64_t row = rr + kr;
      const bool rok = row < rend;
      Ps[kr][c] = (rok && m0 + c < p.M) ? p.P[row * p.ldp + m0 + c] : 0.f;
      Qs[kr][c] = (rok && n0 + c < p.N) ? p.Q[row * p.ldq + n0 + c] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < kTnKR / 2; ++s) {
      const float a = Ps[2 * s + half][wm * 32 + r];
      const float b = Qs[2 * s + half][wn * 32 + r];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
    }
    __syncthreads();
  }
  float* out = p.part + (size_t)split * p.M * p.N;
  const int col = n0 + wn * 32 + r;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int row = m0 + wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * half;
    if (row < p.M && col < p.N) out[(size_t)row * p.N + col] = acc[e];
  }
}

// column sums over row chunks, any width: part[chunk][0..2][n] = sum_r src[r][c] (plain, tcs[r][0]-, tcs[r][1]-
// weighted; tcs NULL: plain only).  A thread owns a column and walks its chunk's rows in order.
__global__ __launch_bounds__(256) void colsum_ragged_kernel(const float* __restrict__ src, int ld, int n, int64_t R,
                                                            int64_t chunk, const float* __restrict__ tcs,
                                                            float* __restrict__ part) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  const int64_t rb = (int64_t)blockIdx.y * chunk;
  const int64_t re = rb + chunk < R ? rb + chunk : R;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  for (int64_t rr = rb; rr < re; ++rr) {
    const float v = src[rr * ld + c];
    s0 += v;
    if (tcs) {
      s1 += tcs[2 * rr] * v;
      s2 += tcs[2 * rr + 1] * v;
    }
  }
  float* o = part + (size_t)blockIdx.y * 3 * n;
  o[c] = s0;
  o[n + c] = s1;
  o[2 * n + c] = s2;
}

// out[i] = sum_s src[s * stride + i], s ascending (fixed order)
__global__ __launch_bounds__(256) void sum_parts_kernel(const float* __restrict__ src, int S, int64_t stride,
                                                        int64_t count, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  float t = 0.f;
  for (int s = 0; s < S; ++s) t += src[(size_t)s * stride + i];
  out[i] = t;
}

// ---------------------------------------------------------------------------------------------------------------
// host side
static int lt_tn_splits(int mt, int nt, int64_t R) {
  // about two workgroups per CU over the tiles, at least 256 rows per split
  const int64_t s = 512 / ((int64_t)mt * nt) > 1 ? 512 / ((int64_t)mt * nt) : 1;
  const int64_t maxs = ceil_div(R, 256) > 1 ? ceil_div(R, 256) : 1;
  return (int)hmin(s, maxs);
}
static int lt_colsum_chunks(int64_t R) { return (int)hmin(512, R / 128 > 1 ? R / 128 : 1); }

struct TnPlan { int mt, nt, splits; int64_t chunk; };
static TnPlan tn_plan(int M, int N, int64_t R) {
  TnPlan t;
  t.mt = (int)ceil_div(M, kTnBM);
  t.nt = (int)ceil_div(N, kTnBN);
  const int s = lt_tn_splits(t.mt, t.nt, R);
  t.chunk = (int64_t)align_up((size_t)ceil_div(R, s), kTnKR);
  t.splits = (int)ceil_div(R, t.chunk);
  return t;
}

static size_t tn_part_floats(int M, int N, int64_t R) { return (size_t)tn_plan(M, N, R).splits * M * N; }
static size_t colsum_part_floats(int n, int64_t R) { return (size_t)lt_colsum_chunks(R) * 3 * n; }

static int launch_tn(const float* P, int M, const float* Q, int N, int64_t R, float* part, float* out,
                     hipStream_t s) {
  const TnPlan t = tn_plan(M, N, R);
  TnRaggedArgs a{};
  a.P = P; a.ldp = M; a.M = M; a.Q = Q; a.ldq = N; a.N = N; a.R = R; a.chunk = t.chunk; a.part = part;
  a.mt = t.mt; a.nt = t.nt;
  hipLaunchKernelGGL(tn_ragged_kernel, dim3((unsigned)(t.mt * t.nt * t.splits)), dim3(256), 0, s, a);
  L2HMC_CHECK_LAUNCH("tn_ragged");
  const int64_t count = (int64_t)M * N;
  hipLaunchKernelGGL(sum_parts_kernel, dim3((unsigned)ceil_div(count, 256)), dim3(256), 0, s, part, t.splits, count,
                     count, out);
  L2HMC_CHECK_LAUNCH("sum_parts (tn)");
  return L2HMC_OK;
}

// column sums of src[R][ld] columns [0, n) -> out_plain [n] (and with tcs: out_cos, out_sin [n])
static int launch_colsum(const float* src, int ld, int n, int64_t R, const float* tcs, float* part, float* out_plain,
                         float* out_cos, float* out_sin, hipStream_t s) {
  const int S = lt_colsum_chunks(R);
  const int64_t chunk = ceil_div(R, S);
  hipLaunchKernelGGL(colsum_ragged_kernel, dim3((unsigned)ceil_div(n, 256), (unsigned)S), dim3(256), 0, s, src, ld, n,
                     R, chunk, tcs, part);
  L2HMC_CHECK_LAUNCH("colsum_ragged");
  float* outs[3] = {out_plain, out_cos, out_sin};
  for (int k = 0; k < (tcs ? 3 : 1); ++k) {
    hipLaunchKernelGGL(sum_parts_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, part + (size_t)k * n, S,
                       (int64_t)3 * n, (int64_t)n, outs[k]);
    L2HMC_CHECK_LAUNCH("sum_parts (colsum)");
  }
  return L2HMC_OK;
}

static int check_widths(const l2hmc_dense_net* net, const char* what) {
  L2HMC_REQUIRE(net != nullptr, "%s: NULL net", what);
  L2HMC_REQUIRE(net->D > 0 && net->H > 0 && net->Ka > 0 && net->Kb > 0,
                "%s: widths (D=%d, Ka=%d, Kb=%d, H=%d) must be positive", what, net->D, net->Ka, net->Kb, net->H);
  return L2HMC_OK;
}

}  // namespace l2hmc

using namespace l2hmc;

extern "C" int l2hmc_stq_dense_taped(const l2hmc_dense_net* net, const float* a, const float* b, const float* bmask,
                                     float t_cos, float t_sin, int64_t rows, float* S, float* T, float* Q, float* h1,
                                     float* h2, l2hmc_stream_t stream) {
  if (int e = check_widths(net, "stq_dense_taped")) return e;
  L2HMC_REQUIRE(rows >= 0, "stq_dense_taped: rows = %lld < 0", (long long)rows);
  if (rows == 0) return L2HMC_OK;
  L2HMC_REQUIRE(a && b && S && T && Q && h1 && h2, "stq_dense_taped: NULL pointer");
  L2HMC_REQUIRE(net->w1_t && net->wt && net->b1 && net->wh_t && net->bh && net->whd_t && net->bhd && net->coeff_s &&
                    net->coeff_q,
                "stq_dense_taped: NULL weight pointer");
  // the launches of l2hmc_stq_dense (leapfrog.hip), activations to the caller's buffers instead of the workspace
  hipStream_t s = (hipStream_t)stream;
  GemmReluArgs l1{};
  l1.A1 = a; l1.lda1 = net->Ka; l1.K1 = net->Ka;
  l1.A2 = b; l1.lda2 = net->Kb;
  l1.cmask_f = bmask; l1.cmask_b = bmask;
  l1.Wt = net->w1_t; l1.K = net->Ka + net->Kb; l1.N = net->H;
  l1.bias = net->b1; l1.wt0 = net->wt; l1.wt1 = net->wt + net->H;
  l1.tc_f = l1.tc_b = t_cos; l1.ts_f = l1.ts_b = t_sin;
  l1.out = h1; l1.ldo = net->H; l1.rows = rows;
  if (int e = launch_gemm_relu(l1, s)) return e;
  GemmReluArgs l2{};
  l2.A1 = h1; l2.lda1 = net->H; l2.K1 = net->H;
  l2.Wt = net->wh_t; l2.K = net->H; l2.N = net->H;
  l2.bias = net->bh; l2.out = h2; l2.ldo = net->H; l2.rows = rows;
  if (int e = launch_gemm_relu(l2, s)) return e;
  HeadsArgs h{};
  h.A = h2; h.lda = net->H; h.K = net->H;
  h.Wt = net->whd_t; h.bhd = net->bhd; h.cs = net->coeff_s; h.cq = net->coeff_q;
  h.q_tanh = net->q_tanh; h.D = net->D; h.rows = rows; h.mode = 0;
  h.S = S; h.T = T; h.Q = Q;
  return launch_heads(h, s);
}

extern "C" int l2hmc_lf_update_v_vjp(const float* v, const float* grad, const float* S, const float* T, const float* Q,
                                     float eps, int32_t dir, int64_t rows, int32_t D, const float* dv_out,
                                     const float* dlogdet, float* dv, float* dgrad, float* dS, float* dT, float* dQ,
                                     float* deps, l2hmc_stream_t stream) {
  L2HMC_REQUIRE(rows >= 0 && D > 0 && (dir == 0 || dir == 1), "lf_update_v_vjp: bad arguments (rows=%lld, D=%d, dir=%d)",
                (long long)rows, D, dir);
  if (rows == 0) return L2HMC_OK;
  L2HMC_REQUIRE(v && grad && S && T && Q && dv_out && dv && dgrad && dS && dT && dQ && deps,
                "lf_update_v_vjp: NULL pointer");
  hipLaunchKernelGGL(lf_update_v_vjp_kernel, dim3((unsigned)ceil_div(rows, 4)), dim3(256), 0, (hipStream_t)stream, v,
                     grad, S, T, Q, eps, dir, rows, D, dv_out, dlogdet, dv, dgrad, dS, dT, dQ, deps);
  L2HMC_CHECK_LAUNCH("lf_update_v_vjp");
  return L2HMC_OK;
}

extern "C" int l2hmc_lf_update_x_vjp(const float* x, const float* v, const float* keep, const float* S, const float* T,
                                     const float* Q, float eps, int32_t dir, int64_t rows, int32_t D,
                                     const float* dx_out, const float* dlogdet, float* dx, float* dv, float* dS,
                                     float* dT, float* dQ, float* deps, l2hmc_stream_t stream) {
  L2HMC_REQUIRE(rows >= 0 && D > 0 && (dir == 0 || dir == 1), "lf_update_x_vjp: bad arguments (rows=%lld, D=%d, dir=%d)",
                (long long)rows, D, dir);
  if (rows == 0) return L2HMC_OK;
  L2HMC_REQUIRE(x && v && keep && S && T && Q && dx_out && dx && dv && dS && dT && dQ && deps,
                "lf_update_x_vjp: NULL pointer");
  hipLaunchKernelGGL(lf_update_x_vjp_kernel, dim3((unsigned)ceil_div(rows, 4)), dim3(256), 0, (hipStream_t)stream, x,
                     v, keep, S, T, Q, eps, dir, rows, D, dx_out, dlogdet, dx, dv, dS, dT, dQ, deps);
  L2HMC_CHECK_LAUNCH("lf_update_x_vjp");
  return L2HMC_OK;
}

extern "C" int l2hmc_lf_update_x_ncp_vjp(const float* x, const float* v, const float* keep, const float* S,
                                         const float* T, const float* Q, float eps, int32_t dir, int64_t rows, int32_t D,
                                         const float* dx_out, const float* dlogdet, float* dx, float* dv, float* dS,
                                         float* dT, float* dQ, float* deps, l2hmc_stream_t stream) {
  L2HMC_REQUIRE(rows >= 0 && D > 0 && (dir == 0 || dir == 1),
                "lf_update_x_ncp_vjp: bad arguments (rows=%lld, D=%d, dir=%d)", (long long)rows, D, dir);
  if (rows == 0) return L2HMC_OK;
  L2HMC_REQUIRE(x && v && keep && S && T && Q && dx_out && dx && dv && dS && dT && dQ && deps,
                "lf_update_x_ncp_vjp: NULL pointer");
  hipLaunchKernelGGL(lf_update_x_ncp_vjp_kernel, dim3((unsigned)ceil_div(rows, 4)), dim3(256), 0, (hipStream_t)stream,
                     x, v, keep, S, T, Q, eps, dir, rows, D, dx_out, dlogdet, dx, dv, dS, dT, dQ, deps);
  L2HMC_CHECK_LAUNCH("lf_update_x_ncp_vjp");
  return L2HMC_OK;
}

extern "C" size_t l2hmc_dense_backward_data_ws_bytes(const l2hmc_dense_net* net) {
  if (!net || net->D <= 0 || net->H <= 0 || net->Ka <= 0 || net->Kb <= 0) return 0;
  const size_t H = net->H;
  return align_up(sizeof(float) * 3 * net->D * H, 256) + align_up(sizeof(float) * H * H, 256) +
         align_up(sizeof(float) * (size_t)(net->Ka + net->Kb) * H, 256);
}

extern "C" int l2hmc_dense_backward_data(const l2hmc_dense_net* net, const float* S, const float* Q, const float* dS,
                                         const float* dT, const float* dQ, const float* h1, const float* h2,
                                         int64_t rows, float* dpre, float* dsq, float* dz2, float* dz1, float* din,
                                         void* ws, size_t ws_bytes, l2hmc_stream_t stream) {
  if (int e = check_widths(net, "dense_backward_data")) return e;
  L2HMC_REQUIRE(rows >= 0, "dense_backward_data: rows = %lld < 0", (long long)rows);
  if (rows == 0) return L2HMC_OK;
  L2HMC_REQUIRE(S && Q && dS && dT && dQ && h1 && h2 && dpre && dz2 && dz1 && din && ws,
                "dense_backward_data: NULL pointer");
  L2HMC_REQUIRE(net->w1_t && net->wh_t && net->whd_t && net->coeff_s && net->coeff_q,
                "dense_backward_data: NULL weight pointer");
  const size_t need = l2hmc_dense_backward_data_ws_bytes(net);
  if (ws_bytes < need) {
    set_error("dense_backward_data: workspace %zu < %zu bytes", ws_bytes, need);
    return L2HMC_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  const int D = net->D, H = net->H, Kin = net->Ka + net->Kb;
  char* base = static_cast<char*>(ws);
  float* whd_n = reinterpret_cast<float*>(base);                                    // [H][3D]
  float* wh_n = reinterpret_cast<float*>(base + align_up(sizeof(float) * 3 * D * (size_t)H, 256));   // [H_in][H_out]
  float* w1_n = reinterpret_cast<float*>(reinterpret_cast<char*>(wh_n) + align_up(sizeof(float) * (size_t)H * H, 256));
  hipLaunchKernelGGL(lt_transpose_kernel, dim3((unsigned)ceil_div(H, 32), (unsigned)ceil_div(3 * D, 32)), dim3(256), 0,
                     s, net->whd_t, 3 * D, H, whd_n);
  L2HMC_CHECK_LAUNCH("transpose whd");
  hipLaunchKernelGGL(lt_transpose_kernel, dim3((unsigned)ceil_div(H, 32), (unsigned)ceil_div(H, 32)), dim3(256), 0, s,
                     net->wh_t, H, H, wh_n);
  L2HMC_CHECK_LAUNCH("transpose wh");
  hipLaunchKernelGGL(lt_transpose_kernel, dim3((unsigned)ceil_div(Kin, 32), (unsigned)ceil_div(H, 32)), dim3(256), 0,
                     s, net->w1_t, H, Kin, w1_n);
  L2HMC_CHECK_LAUNCH("transpose w1");
  const int64_t n = rows * D;
  hipLaunchKernelGGL(heads_pre_bwd_kernel, dim3((unsigned)hmin(ceil_div(n, 256), 4096)), dim3(256), 0, s, S, Q, dS, dT,
                     dQ, net->coeff_s, net->coeff_q, net->q_tanh, rows, D, dpre, dsq);
  L2HMC_CHECK_LAUNCH("heads_pre_bwd");
  // dz2 = (dpre . Whd) gated by h2 > 0
  GemmReluArgs g2{};
  g2.kind = 3;
  g2.A1 = dpre; g2.lda1 = 3 * D; g2.K1 = 3 * D; g2.K = 3 * D;
  g2.Wt = whd_n; g2.N = H;
  g2.gate = h2; g2.ldg = H;
  g2.out = dz2; g2.ldo = H; g2.rows = rows;
  if (int e = launch_gemm_relu(g2, s)) return e;
  // dz1 = (dz2 . Wh) gated by h1 > 0
  GemmReluArgs g1{};
  g1.kind = 3;
  g1.A1 = dz2; g1.lda1 = H; g1.K1 = H; g1.K = H;
  g1.Wt = wh_n; g1.N = H;
  g1.gate = h1; g1.ldg = H;
  g1.out = dz1; g1.ldo = H; g1.rows = rows;
  if (int e = launch_gemm_relu(g1, s)) return e;
  // din = dz1 . W1 = [da | db]
  GemmReluArgs g0{};
  g0.kind = 4;
  g0.A1 = dz1; g0.lda1 = H; g0.K1 = H; g0.K = H;
  g0.Wt = w1_n; g0.N = Kin;
  g0.out = din; g0.ldo = Kin; g0.rows = rows;
  return launch_gemm_relu(g0, s);
}

extern "C" size_t l2hmc_dense_weight_grads_ws_bytes(const l2hmc_dense_net* net, int64_t R) {
  if (!net || net->D <= 0 || net->H <= 0 || net->Ka <= 0 || net->Kb <= 0 || R < 0) return 0;
  if (R == 0) return 256;
  const int D = net->D, H = net->H, Kin = net->Ka + net->Kb;
  size_t f = tn_part_floats(H, Kin, R);
  f = f > tn_part_floats(H, H, R) ? f : tn_part_floats(H, H, R);
  f = f > tn_part_floats(3 * D, H, R) ? f : tn_part_floats(3 * D, H, R);
  const int nmax = hmax(H, 3 * D);
  f = f > colsum_part_floats(nmax, R) ? f : colsum_part_floats(nmax, R);
  return align_up(sizeof(float) * f, 256);
}

extern "C" int l2hmc_dense_weight_grads(const l2hmc_dense_net* net, int64_t R, const float* in, const float* h1,
                                        const float* h2, const float* dz1, const float* dz2, const float* dpre,
                                        const float* dsq, const float* tcs, const l2hmc_dense_grads* g, void* ws,
                                        size_t ws_bytes, l2hmc_stream_t stream) {
  if (int e = check_widths(net, "dense_weight_grads")) return e;
  L2HMC_REQUIRE(R >= 0, "dense_weight_grads: R = %lld < 0", (long long)R);
  L2HMC_REQUIRE(g && g->w1_t && g->wt && g->b1 && g->wh_t && g->bh && g->whd_t && g->bhd && g->coeff_s && g->coeff_q,
                "dense_weight_grads: NULL gradient pointer");
  hipStream_t s = (hipStream_t)stream;
  const int D = net->D, H = net->H, Kin = net->Ka + net->Kb;
  if (R == 0) {      // an empty contraction: every gradient is 0
    const struct { float* p; size_t n; } z[] = {{g->w1_t, (size_t)H * Kin}, {g->wt, 2 * (size_t)H}, {g->b1, (size_t)H},
                                                 {g->wh_t, (size_t)H * H}, {g->bh, (size_t)H}, {g->whd_t, 3 * (size_t)D * H},
                                                 {g->bhd, 3 * (size_t)D}, {g->coeff_s, (size_t)D}, {g->coeff_q, (size_t)D}};
    for (const auto& e : z)
      if (hipMemsetAsync(e.p, 0, sizeof(float) * e.n, s) != hipSuccess) {
        set_error("dense_weight_grads: hipMemsetAsync failed");
        return L2HMC_ERR_HIP;
      }
    return L2HMC_OK;
  }
  L2HMC_REQUIRE(in && h1 && h2 && dz1 && dz2 && dpre && dsq && tcs && ws, "dense_weight_grads: NULL pointer");
  const size_t need = l2hmc_dense_weight_grads_ws_bytes(net, R);
  if (ws_bytes < need) {
    set_error("dense_weight_grads: workspace %zu < %zu bytes", ws_bytes, need);
    return L2HMC_ERR_WORKSPACE;
  }
  float* part = static_cast<float*>(ws);
  // first layer: w1_t [H][Ka+Kb] = dz1^T . [a | b]; b1 = sum dz1; wt = (sum cos dz1, sum sin dz1)
  if (int e = launch_tn(dz1, H, in, Kin, R, part, g->w1_t, s)) return e;
  if (int e = launch_colsum(dz1, H, H, R, tcs, part, g->b1, g->wt, g->wt + H, s)) return e;
  // hidden layer: wh_t [H_out][H_in] = dz2^T . h1; bh = sum dz2
  if (int e = launch_tn(dz2, H, h1, H, R, part, g->wh_t, s)) return e;
  if (int e = launch_colsum(dz2, H, H, R, nullptr, part, g->bh, nullptr, nullptr, s)) return e;
  // heads: whd_t [3D][H] = dpre^T . h2; bhd = sum dpre
  if (int e = launch_tn(dpre, 3 * D, h2, H, R, part, g->whd_t, s)) return e;
  if (int e = launch_colsum(dpre, 3 * D, 3 * D, R, nullptr, part, g->bhd, nullptr, nullptr, s)) return e;
  // coefficients: sum dS S, sum dQ Q
  if (int e = launch_colsum(dsq, 2 * D, D, R, nullptr, part, g->coeff_s, nullptr, nullptr, s)) return e;
  return launch_colsum(dsq + D, 2 * D, D, R, nullptr, part, g->coeff_q, nullptr, nullptr, s);
}
