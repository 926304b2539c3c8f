/*
 * l2hmc_hip.h -- C ABI of libl2hmc_hip.so: the MI355X (gfx950) implementation
 * of the L2HMC augmented-leapfrog hot path of saforem2/l2hmc.
 *
 * Drop-in boundary.  The reference is pure Python on TensorFlow 1.x; its "FFI"
 * for this path is the set of TF graph ops its Dynamics classes emit.  Each
 * entry point below replaces the ops of the reference function cited next to
 * it (paths relative to the reference checkout, `l2hmc/...`).  The Python host
 * classes in l2hmc_amd/ (GaugeDynamics, Dynamics, propose, ...) bind these via
 * ctypes; INTEGRATION.md shows the stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous fp32 (int32 where said);
 *     rows are chains (or chain x direction pairs), row-major [rows][D];
 *   - nothing allocates, frees or synchronises: work is enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the default stream); scratch
 *     comes from the caller through (ws, ws_bytes), sized by the *_ws_bytes
 *     queries, so calls are hipGraph-capturable; a workspace's content on
 *     entry is arbitrary and is not preserved (no entry reads what an earlier
 *     call left there, but a train_backward its train_forward's tape): only
 *     the documented ticket words of step_sums must be zero on entry;
 *   - inputs are never written; outputs never alias inputs unless documented;
 *   - return value: L2HMC_OK or an error code; l2hmc_last_error() gives text.
 *     Shape/argument violations are rejected on the host before any launch;
 *   - randomness is always an input buffer (l2hmc_fill_* produce them), so a
 *     caller can replay the reference's draws;
 *   - direction codes: 0 = forward (_forward_lf), 1 = backward (_backward_lf).
 */
#ifndef L2HMC_HIP_H
#define L2HMC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define L2HMC_OK 0
#define L2HMC_ERR_ARG 1       /* bad shape / null pointer / unsupported size */
#define L2HMC_ERR_HIP 2       /* a HIP runtime call or launch failed */
#define L2HMC_ERR_WORKSPACE 3 /* workspace too small */

#define L2HMC_ABI_VERSION 1

typedef void* l2hmc_stream_t;

int l2hmc_abi_version(void);
const char* l2hmc_last_error(void);

/* ------------------------------------------------------------------------
 * U(1) lattice: action, force, observables.
 *   lattice/lattice.py:337-362 total_action; :285-313 calc_plaq_observables;
 *   gauge_model.py:659-725 _calc_plaq_sums/_total_actions/_avg_plaqs/_top_charges;
 *   dynamics/gauge_dynamics.py:698-709 grad_potential (autodiff of the action;
 *   closed form in lattice/gauge_lattice.py:427-459).
 * x: [rows][T][X][2].  Any output pointer may be NULL (skipped).
 *   action[r]  = sum_ij (1 - cos P)          force[r][:] = beta * dS/dx
 *   avg_plaq[r]= sum_ij cos P / (T*X)        top_charge[r] = sum_ij project(P) / 2pi
 * ------------------------------------------------------------------------ */
int l2hmc_u1_action_force(const float* x, int64_t rows, int32_t T, int32_t X, float beta,
                          float* action, float* force, float* avg_plaq, float* top_charge,
                          l2hmc_stream_t stream);

/* gauge_model.py:659-681: plaq[r][i][j] = x0[i,j] - x1[i,j] - x0[i,j+1] + x1[i+1,j]. */
int l2hmc_u1_plaq_sums(const float* x, int64_t rows, int32_t T, int32_t X, float* plaq,
                       l2hmc_stream_t stream);

/* gauge_model.py:1180,1388: samples = np.mod(x_out, 2*pi) between MCMC steps, done on the device
 * (fp32, result in [0, 2*pi)).  out may alias x. */
int l2hmc_wrap_angle(const float* x, int64_t n, float* out, l2hmc_stream_t stream);

/* gauge_dynamics.py:683-689 / utils/dynamics.py:112-113: out[r] = 0.5 * sum_d v^2. */
int l2hmc_kinetic_energy(const float* v, int64_t rows, int32_t D, float* out, l2hmc_stream_t stream);

/* ------------------------------------------------------------------------
 * Dense S/T/Q network (GenericNet / dense trunk of ConvNet3D / `network` MLP).
 *   network/generic_net.py:129-146, network/conv_net.py:264-280,
 *   utils/network.py:89-114.
 * Weights are PACKED by the host (l2hmc_amd/network.py) from the reference's
 * [in,out] Dense kernels into k-contiguous ("[out][in]") device buffers:
 *   w1_t   [H][Ka+Kb]  rows of v_layer (first input, Ka cols) then x_layer (Kb)
 *   wt     [2][H]      t_layer kernel            b1 [H] = b_v + b_x + b_t
 *   wh_t   [H][H]      h_layer                   bh [H]
 *   whd_t  [3][D][H]   scale / translation / transformation layers
 *   bhd    [3][D]      their biases
 *   coeff_s, coeff_q [D]  coeff_scale / coeff_transformation (exp applied on device)
 *   q_tanh: 0 = GenericNet/ConvNet3D (no tanh on transformation, quirk Q1),
 *           1 = utils/network.py `network` (ScaleTanh on F as well).
 * Shapes (generic_net.py:20-93 accepts any x_dim / num_hidden):
 *   - the layer-by-layer kernels (l2hmc_stq_dense, every l2hmc_gauge_* entry point) take ANY positive D, H, Ka, Kb
 *     and any lattice T x X; widths that are multiples of 32 with 16-byte aligned rows take the staged 16-byte
 *     loads, everything else (6x6: D = 72, H = 288; 3x5: D = 30) a bounds-checked instantiation of the same
 *     kernels -- identical arithmetic, slower loads;
 *   - the whole-trajectory kernels exist for D = 128 (T*X = 64, X a power of two): GenericNet H = 512 and
 *     ConvNet3D F = 8 / H = 256; other shapes run layer by layer (l2hmc_dense_pack_bytes() == 0 says which);
 *     plans with hmc = 1 have one for any lattice of up to 1024 sites;
 *   - the TRAINING entry points (l2hmc_gauge_train_*) need D, H, Ka, Kb multiples of 32; GaugeTrainer trains
 *     GenericNet plans of other widths through the layered-training entries below (l2hmc_stq_dense_taped, ...,
 *     l2hmc_u1_force_hvp);
 *   - ConvNet3D needs T and X multiples of 4 (two 2x2 poolings) and filter sizes (3,3,2), (2,2,2).
 * ------------------------------------------------------------------------ */
typedef struct l2hmc_dense_net {
  int32_t D;   /* output width (x_dim) */
  int32_t H;   /* hidden width */
  int32_t Ka;  /* width of first input  (v_layer / embed_1) */
  int32_t Kb;  /* width of second input (x_layer / embed_2) */
  const float* w1_t;
  const float* wt;
  const float* b1;
  const float* wh_t;
  const float* bh;
  const float* whd_t;
  const float* bhd;
  const float* coeff_s;
  const float* coeff_q;
  int32_t q_tanh;
  int32_t reserved;
  const float* packed; /* optional: l2hmc_dense_pack() image for the fused trajectory kernel, or NULL */
} l2hmc_dense_net;

/* Fragment-ordered copy of (w1_t, wh_t, whd_t) for the whole-trajectory kernel:
 * [wave][k-chunk][n-tile][lane][4] per layer, so every B-operand load of a wave is
 * one contiguous 1 KiB read.  GenericNet plans get a second image behind it for the
 * kernel's sub-tile form ([wave][k-chunk][64-column block][4][lane][4]; batches that cannot
 * put a 16-row tile on every CU run 4 / 8 / 12 rows per workgroup, bit-identical results).
 * pack_bytes() is 0 when the shape has no fused kernel (then leave .packed NULL: the
 * layer-by-layer kernels are used).  Re-pack after every weight update. */
size_t l2hmc_dense_pack_bytes(const l2hmc_dense_net* net);
int l2hmc_dense_pack(const l2hmc_dense_net* net, float* packed, l2hmc_stream_t stream);

/* Convolutional front-end of ConvNet3D, channels_last (network/conv_net.py:90-164, 247-262):
 * per network input Conv3D(F,(3,3,2),same,relu) -> MaxPool3D(2,2,'same') -> Conv3D(2F,(2,2,2),same,relu)
 * -> MaxPool3D -> flatten to nflat = (T/4)*(X/4)*2F features, which feed the dense trunk above with
 * Ka = Kb = nflat.  Kernels are passed in the Keras layout [k0][k1][k2][Cin][Cout] unchanged.
 *   *_a: first input  (conv_v1 / conv_v2)      *_b: second input (conv_x1 / conv_x2)              */
typedef struct l2hmc_conv3d_front {
  int32_t F;          /* num_filters (gauge_dynamics.py:130: space_size) */
  int32_t reserved;
  const float* w1_a; const float* b1_a; const float* w2_a; const float* b2_a;
  const float* w1_b; const float* b1_b; const float* w2_b; const float* b2_b;
} l2hmc_conv3d_front;

/* scratch for one net evaluation on `rows` rows: two [rows][H] activations */
size_t l2hmc_stq_ws_bytes(int64_t rows, int32_t H);

/* (S, T, Q) = net([a, b * bmask, t])  with t = [t_cos, t_sin] for every row.
 * a: [rows][Ka], b: [rows][Kb], bmask: [Kb] or NULL.  S, T, Q: [rows][D]. */
int l2hmc_stq_dense(const l2hmc_dense_net* net, const float* a, const float* b, const float* bmask,
                    float t_cos, float t_sin, int64_t rows, float* S, float* T, float* Q,
                    void* ws, size_t ws_bytes, l2hmc_stream_t stream);

/* ConvNet3D.call (network/conv_net.py:247-280) on lattice inputs a, b: [rows][2*T*X]. */
size_t l2hmc_stq_conv3d_ws_bytes(int64_t rows, int32_t H, int32_t T, int32_t X, int32_t F);
int l2hmc_stq_conv3d(const l2hmc_conv3d_front* front, const l2hmc_dense_net* net, int32_t T, int32_t X,
                     const float* a, const float* b, const float* bmask, float t_cos, float t_sin,
                     int64_t rows, float* S, float* Tr, float* Q, void* ws, size_t ws_bytes,
                     l2hmc_stream_t stream);

/* ------------------------------------------------------------------------
 * Leapfrog sub-updates on materialised S/T/Q (standalone forms).
 *   v: gauge_dynamics.py:486-508 (dir 0), :537-561 (dir 1)
 *   x: gauge_dynamics.py:511-534 (dir 0), :565-590 (dir 1);
 *      `keep` is the mask fed to the net (1 = element kept, 0 = updated).
 * logdet[r] receives sum_d s (v) or sum_d (1-keep) s (x).  out may alias in.
 * ------------------------------------------------------------------------ */
int l2hmc_lf_update_v(const float* v, const float* grad, const float* S, const float* T,
                      const float* Q, float eps, int32_t dir, int64_t rows, int32_t D,
                      float* v_out, float* logdet, l2hmc_stream_t stream);
int l2hmc_lf_update_x(const float* x, const float* v, const float* keep, const float* S,
                      const float* T, const float* Q, float eps, int32_t dir, int64_t rows,
                      int32_t D, float* x_out, float* logdet, l2hmc_stream_t stream);

/* Position sub-update of the torus-exact mode (L2HMC_PLAN_PERIODIC; no reference counterpart).  With e_s = exp(+-eps S)
 * (+ dir 0, - dir 1), drift = eps (exp(eps Q) v + T) and w = x (dir 0) or x - drift (dir 1):
 *   y = 2 atan2(e_s sin(w / 2), cos(w / 2)) [+ drift for dir 0],   x' = keep x + (1 - keep) y,
 *   logdet[r] = sum_d (1 - keep) (+-eps S - log(cos^2(w / 2) + e_s^2 sin^2(w / 2))).
 * atan2 takes its principal value, so x' is defined modulo 2 pi.  S, T, Q may be NULL (= 0); out may alias in. */
int l2hmc_lf_update_x_ncp(const float* x, const float* v, const float* keep, const float* S,
                          const float* T, const float* Q, float eps, int32_t dir, int64_t rows,
                          int32_t D, float* x_out, float* logdet, l2hmc_stream_t stream);

/* out[r] = [cos x[r] | sin x[r]] ([rows][2D]) for x [rows][D]: the form in which the networks of a periodic plan see
 * the link angles.  _vjp: dx[r][c] += -sin x[r][c] dfeat[r][c] + cos x[r][c] dfeat[r][D + c], dfeat with row stride
 * ldf >= 2D (a slice of a wider cotangent).  Any D; 16-byte accesses when D (and ldf) are multiples of 4 and the
 * bases aligned. */
int l2hmc_u1_angle_features(const float* x, int64_t rows, int32_t D, float* out, l2hmc_stream_t stream);
int l2hmc_u1_angle_features_vjp(const float* x, const float* dfeat, int64_t ldf, int64_t rows, int32_t D, float* dx,
                                l2hmc_stream_t stream);

/* gauge_dynamics.py:592-609 / utils/dynamics.py:312-319:
 * p = exp(min(h_old - h_new + sumlogdet, 0)), non-finite -> 0. */
int l2hmc_accept_prob(const float* h_old, const float* h_new, const float* sumlogdet, int64_t n,
                      float* p, l2hmc_stream_t stream);

/* gauge_dynamics.py:221-257 (strict=1: accept iff p > u, forward iff coin > 0.5)
 * utils/sampler.py:33-59    (strict=0: accept iff p - u >= 0, forward iff coin != 0).
 * xf,vf,pf / xb,vb,pb: forward / backward trajectories of the same B chains. */
int l2hmc_mix_accept(const float* x, const float* xf, const float* vf, const float* pf,
                     const float* xb, const float* vb, const float* pb, const float* coin,
                     const float* u, int32_t strict, int64_t B, int32_t D, float* x_prop,
                     float* v_prop, float* p, float* x_out, l2hmc_stream_t stream);

/* ------------------------------------------------------------------------
 * Lattice integrator: gauge_dynamics.py:412-483 (_forward_lf/_backward_lf),
 * :261-313 (transition_kernel), :195-259 (apply_transition).
 * ------------------------------------------------------------------------ */
#define L2HMC_PLAN_LAYERED 1   /* never use the fused whole-trajectory kernel */
#define L2HMC_PLAN_CONV3D 2    /* nets are ConvNet3D: xfront / vfront are set, nets have Ka = Kb = nflat */
#define L2HMC_PLAN_SELECTED_ONLY 4   /* l2hmc_gauge_mcmc_step integrates only the direction each chain's coin picks:
                                      * same draws, same outputs as the default whenever the other direction is
                                      * finite (the reference multiplies it by an exact 0), half the work */
#define L2HMC_PLAN_RECOMPUTE 8       /* layer-by-layer path: form every first-layer product anew, as the reference's graph
                                      * does, instead of keeping the ones a leapfrog step repeats (XNet's product with
                                      * the momentum across the two position sub-updates; VNet's whole product from the
                                      * end of one step to the start of the next).  Same bits either way; diagnostic */
#define L2HMC_PLAN_TILES16_ONLY 16   /* whole-trajectory kernel: every batch on the 16-row form (no sub-tile form, no 32-row
                                      * form, no launch split).  All forms give the same bits; A/B and the bit-identity test */
#define L2HMC_PLAN_ALL_COLUMNS 32    /* a position sub-update forms S / T / Q for EVERY column, as the reference's graph
                                      * does, instead of only the columns its mask lets move: on the layer-by-layer path,
                                      * and in the whole-step kernel with plan.heads set (identical x, v for finite
                                      * trajectories; 0 x non-finite differs: DESIGN.md D1).  A/B switch */
#define L2HMC_PLAN_FULL_L1 64        /* whole-step kernel with plan.heads set: a position sub-update forms XNet's first-layer
                                      * product with keep (.) x over all D columns instead of the D / 2 it keeps (same bits;
                                      * the active-column heads stay on; L2HMC_PLAN_ALL_COLUMNS switches off both).  A/B switch */
#define L2HMC_PLAN_SINGLE_KICKS 128  /* whole-step kernel, 16-row GenericNet sampling form: the second momentum half-kick of a
                                      * leapfrog step and the first of the next one stay two network calls instead of one
                                      * pass over two time slices (same bits).  A/B switch */
#define L2HMC_PLAN_PERIODIC 256      /* torus-exact L2HMC (GenericNet only; ignored with hmc = 1): the networks see every link
                                      * angle through [cos x | sin x] -- VNet has Ka = 2D, Kb = D (its first input is x),
                                      * XNet has Ka = D, Kb = 2D (its second input is the masked x, the mask applied to both
                                      * halves) -- and the position sub-update is l2hmc_lf_update_x_ncp, a map of the circle
                                      * onto itself.  The proposal then commutes with 2 pi shifts of any link, so the wrap
                                      * between MCMC steps is harmless and the chain exact for any weights.  Runs layer by
                                      * layer, every first-layer product formed anew: l2hmc_gauge_plan_fused() == 0 (unless
                                      * L2HMC_PLAN_PERIODIC_STEP selects the mode's whole-step kernel), and the
                                      * l2hmc_gauge_train_* entries refuse the plan (unless L2HMC_PLAN_PERIODIC_TRAIN is set) */
#define L2HMC_PLAN_PERIODIC_STEP 512 /* with L2HMC_PLAN_PERIODIC only (without it an hmc = 0 plan is refused; ignored with
                                      * hmc = 1; L2HMC_PLAN_LAYERED wins over it): where the plan has the kernel -- GenericNet,
                                      * D = 128 with X a power of two (8x8, 4x16, ...), H = 512, both nets' .packed set -- the
                                      * trajectory, leapfrog, transition-draw and MCMC-step entries run the periodic plan in ONE
                                      * launch (l2hmc_gauge_plan_fused() == 1; a beta ladder in l2hmc_gauge_mcmc_step_ladder
                                      * too), 16 rows per workgroup at every batch size.  Any other plan carries the flag and
                                      * runs layer by layer.  L2HMC_PLAN_RECOMPUTE switches the kept first-layer products of
                                      * that kernel off (same bits); TILES16_ONLY, ALL_COLUMNS, FULL_L1 and SINGLE_KICKS do
                                      * nothing there.  l2hmc_gauge_transition_ladder and the training entries are unchanged */
#define L2HMC_PLAN_PERIODIC_TRAIN 1024 /* with L2HMC_PLAN_PERIODIC only (without it an hmc = 0 plan is refused; ignored with
                                      * hmc = 1): the l2hmc_gauge_train_* entries take the torus-exact plan instead of
                                      * refusing it, layer by layer on the tiled kernels -- GenericNet with D and H multiples
                                      * of 32 (T * X a multiple of 16: 4x4, 2x8, 4x8, 8x8, 16x16, ...), XNet Ka = D, Kb = 2D,
                                      * VNet Ka = 2D, Kb = D; other widths are refused with the widths named.  The taped
                                      * first-layer input of a call is 3D wide, [cos x | sin x | beta force] for VNet and
                                      * [v | keep cos x | keep sin x] for XNet, and the position sub-update and its reverse are
                                      * l2hmc_lf_update_x_ncp's.  Every sampling entry ignores the flag (same bits, same
                                      * l2hmc_gauge_ws_bytes); it composes with L2HMC_PLAN_PERIODIC_STEP.  Workspace: see
                                      * l2hmc_gauge_train_ws_bytes */
#define L2HMC_PLAN_PERIODIC_TAPE 2048 /* with L2HMC_PLAN_PERIODIC and L2HMC_PLAN_PERIODIC_TRAIN only (without both an hmc = 0
                                      * plan is refused; ignored with hmc = 1; L2HMC_PLAN_LAYERED wins over it): where the
                                      * plan has the kernel -- GenericNet, D = 128 with X a power of two (8x8, 4x16, ...),
                                      * H = 512, both nets' .packed set; L2HMC_PLAN_PERIODIC_STEP is not needed and composes
                                      * -- l2hmc_gauge_train_forward and l2hmc_gauge_train_forward_ladder run the plan in ONE
                                      * launch of the mode's whole-trajectory kernel (l2hmc_gauge_plan_train_fused() == 1),
                                      * which writes the tape the layer-by-layer forward writes, in the same layout: `in`
                                      * [3D], `st`, h1, h2 and the S / T / Q planes, next to x_out, v_out, sumlogdet and
                                      * p_accept.  The relu `gate` words of the workspace are NOT written: their only reader
                                      * is the reference mode's fused reverse kernel, and the reverse pass of a torus-exact
                                      * plan stays layer by layer on the tiled kernels, gating on h1 > 0 / h2 > 0.  The
                                      * launch has the bits of the untaped kernel (l2hmc_gauge_trajectory on a
                                      * L2HMC_PLAN_PERIODIC_STEP plan) on the same rows; against the layer-by-layer taped
                                      * forward it differs in rounding (fast exp, another k order).  Any other plan carries
                                      * the flag and runs as without it.  Every sampling entry ignores the flag (same bits,
                                      * same l2hmc_gauge_ws_bytes), and l2hmc_gauge_train_ws_bytes is the same with and
                                      * without it */
typedef struct l2hmc_gauge_plan {
  int32_t T, X;            /* lattice extents; D = 2*T*X */
  int32_t num_steps;       /* N_LF */
  int32_t hmc;             /* 1: S=T=Q=0 (gauge_dynamics.py:102-108), nets ignored: plain HMC.  Lattices of up to 1024
                            * sites run every entry point below in ONE launch (l2hmc_gauge_plan_fused() == 1);
                            * larger ones, and L2HMC_PLAN_LAYERED, go layer by layer */
  float eps;
  int32_t flags;           /* L2HMC_PLAN_* bits */
  const float* masks;      /* [num_steps][D] 0/1, gauge_dynamics.py:651-661 */
  l2hmc_dense_net xnet;    /* position_fn */
  l2hmc_dense_net vnet;    /* momentum_fn */
  l2hmc_conv3d_front xfront;   /* conv layers of position_fn (L2HMC_PLAN_CONV3D only) */
  l2hmc_conv3d_front vfront;   /* conv layers of momentum_fn */
  const void* heads;       /* optional: l2hmc_gauge_pack_heads() image of (masks, xnet), or NULL = every column */
} l2hmc_gauge_plan;

/* Active-column heads of the whole-step kernel (GenericNet D = 128, H = 512 on an 8x8-site lattice; bytes = 0 for
 * other plans).  For every mask row and keep sense it lists the D / 2 columns a position sub-update moves and packs
 * XNet's S / T / Q weights of just those columns; l2hmc_gauge_mcmc_step then forms the heads of its position
 * sub-updates on those columns only (same bits).  It also packs the rows D + c of XNet's first-layer weights for the
 * D / 2 columns c the sub-update KEEPS: its second input keep (.) x is zero everywhere else, so the kernel forms that
 * product over D / 2 k instead of D (same bits; a row in which a moving column holds 0 x non-finite = NaN comes out
 * NaN as before).  Rows whose mask is not exactly D / 2 zeros and D / 2 ones are recorded as such and take every
 * column and the full first layer.  Re-pack after any change of plan.masks or of XNet's weights.
 * Layout (N = num_steps, pair = 2 * mask row + keep sense whose columns move; everything int32 / float32):
 *   int   ok[N][2]             1 = the pair is eligible
 *   int   cols[N][2][D / 2]    the columns the pair moves, ascending (-1 if not eligible)
 *   int   compact_k[N][D]      column -> its k in the first-layer section of the pair that keeps it (-1 if not eligible)
 *   (padding to 256 bytes)
 *   float heads[N][2][4 sections][H / 16 chunks][S | T | Q][64 lanes][4]       3 * (D / 2) * H floats per pair
 *   float l1[N][2][4 sections][D / 32 chunks][H / 64 tiles][64 lanes][4]       (D / 2) * H floats per pair
 * Both images are in the fragment order of the 4-wave weight image (l2hmc_dense_pack): lane = 16 q + r holds column
 * tile * 16 + r, k = chunk * 16 + 4 q + j.  The matrix instruction takes the 16 k of a chunk in the order 4 q + e,
 * e = 0..3 outer, q = 0..3 inner; the n-th kept column in THAT order over all D columns sits at the compact k whose
 * turn is n-th in the same order, so every accumulator adds its kept terms in the order of the full walk. */
size_t l2hmc_gauge_pack_heads_bytes(const l2hmc_gauge_plan* plan);
int l2hmc_gauge_pack_heads(const l2hmc_gauge_plan* plan, void* heads, l2hmc_stream_t stream);

size_t l2hmc_gauge_ws_bytes(const l2hmc_gauge_plan* plan, int64_t rows);

/* Which kernels a plan runs through (no reference counterpart; for callers that report or size by it):
 * 1 = a whole-trajectory kernel exists for this shape and L2HMC_PLAN_LAYERED is not set, 0 = layer by layer,
 * negative = invalid plan (l2hmc_last_error says why). */
int l2hmc_gauge_plan_fused(const l2hmc_gauge_plan* plan);

/* How one MCMC step of a whole-trajectory plan (GenericNet, 8x8) over `rows_all` chain-rows is cut into launches on a
 * device with `cus` compute units (host logic only, no device call, no reference counterpart): writes up to three
 * {rows, rows per workgroup} parts and returns their number.  Rows per workgroup 4 / 8 / 12 = sub-tile form, 16, 32. */
int l2hmc_gauge_step_plan(int64_t rows_all, int32_t cus, int64_t* rows_out, int32_t* rows_per_wg_out);

/* One augmented leapfrog step IN PLACE on x, v: [rows][D]; dir: [rows] int32 per
 * row (0 fwd, 1 bwd), or NULL = all forward.  `step` is the loop counter t of
 * transition_kernel: backward rows use index num_steps-1-step for time and
 * mask, as _backward_lf does internally.  logdet[rows] is ACCUMULATED (+=). */
int l2hmc_gauge_leapfrog(const l2hmc_gauge_plan* plan, float beta, int32_t step, float* x, float* v,
                         const int32_t* dir, int64_t rows, float* logdet, void* ws, size_t ws_bytes,
                         l2hmc_stream_t stream);
/* ... and the steps [step_begin, step_end) of a trajectory in one call (one launch where the plan has a
 * whole-trajectory kernel): 0 <= step_begin < step_end <= num_steps. */
int l2hmc_gauge_leapfrog_steps(const l2hmc_gauge_plan* plan, float beta, int32_t step_begin, int32_t step_end, float* x,
                               float* v, const int32_t* dir, int64_t rows, float* logdet, void* ws, size_t ws_bytes,
                               l2hmc_stream_t stream);

/* Full trajectory of `rows` chain-direction pairs: x0, v0 -> x_out, v_out,
 * sumlogdet, accept probability (any of the last two may be NULL). */
int l2hmc_gauge_trajectory(const l2hmc_gauge_plan* plan, float beta, const float* x0, const float* v0,
                           const int32_t* dir, int64_t rows, float* x_out, float* v_out,
                           float* sumlogdet, float* p_accept, void* ws, size_t ws_bytes,
                           l2hmc_stream_t stream);

/* apply_transition on B chains.  v0_f, v0_b: [B][D] momenta for the two
 * directions; coin, u: [B] uniforms.  both_directions=1 integrates forward AND
 * backward for every chain like the reference and mixes (2B rows); 0 integrates
 * only the direction each chain's coin selects (B rows; identical outputs when
 * the unselected trajectory is finite). Outputs [B][D], [B][D], [B], [B][D]. */
size_t l2hmc_gauge_transition_ws_bytes(const l2hmc_gauge_plan* plan, int64_t B, int32_t both_directions);
int l2hmc_gauge_transition(const l2hmc_gauge_plan* plan, float beta, const float* x, const float* v0_f,
                           const float* v0_b, const float* coin, const float* u, int64_t B,
                           int32_t both_directions, float* x_prop, float* v_prop, float* p_accept,
                           float* x_out, void* ws, size_t ws_bytes, l2hmc_stream_t stream);

/* l2hmc_gauge_transition (the caller's draws) with a beta per chain: chain c reads betas[c * chain_stride], betas a
 * DEVICE pointer, chain_stride 1 (betas [B]) or 0 (one value) -- the convention of l2hmc_gauge_mcmc_step_ladder with
 * chains = B, so rows c and B + c of the stacked [forward; backward] trajectories run at chain c's beta.  The
 * whole-trajectory kernels take one beta, so this entry ALWAYS runs layer by layer, whatever plan->flags says (it
 * runs on a copy of the plan with L2HMC_PLAN_LAYERED set; l2hmc_gauge_mcmc_step_ladder is the one-launch ladder
 * step).  A chain has the bits of l2hmc_gauge_transition on a L2HMC_PLAN_LAYERED plan at its beta.  Everything else is
 * l2hmc_gauge_transition's: arguments, outputs, the workspace of l2hmc_gauge_transition_ws_bytes, B == 0 a no-op after
 * the checks.  Refused with L2HMC_ERR_ARG before any device call: NULL betas, a chain_stride other than 0 or 1,
 * plan->hmc = 1 (l2hmc_gauge_hmc_run_ladder is that path), and everything l2hmc_gauge_transition refuses.  The VALUES
 * of betas are on the device and are not checked; GaugeDynamics.apply_transition checks them. */
int l2hmc_gauge_transition_ladder(const l2hmc_gauge_plan* plan, const float* betas, int64_t chain_stride,
                                  const float* x, const float* v0_f, const float* v0_b, const float* coin,
                                  const float* u, int64_t B, int32_t both_directions, float* x_prop, float* v_prop,
                                  float* p_accept, float* x_out, void* ws, size_t ws_bytes, l2hmc_stream_t stream);

/* apply_transition (gauge_dynamics.py:195-259) with the library's own draws -- Philox streams (seed, 2*draw) for the
 * stacked momenta [v0_f; v0_b] and (seed, 2*draw+1) for coin | u, exactly the layout of l2hmc_gauge_mcmc_step,
 * reproducible with l2hmc_fill_normal/_uniform -- instead of caller-provided ones: what `dynamics(x, beta)` is in
 * the reference.  ONE launch for plans with a whole-trajectory kernel.  ws: l2hmc_gauge_mcmc_step_ws_bytes(plan, B).
 * draw must be below 2^63 (the rule of l2hmc_gauge_mcmc_step; L2HMC_ERR_ARG before any device call, B == 0 included). */
int l2hmc_gauge_transition_draw(const l2hmc_gauge_plan* plan, float beta, const float* x, int64_t B, uint64_t seed,
                                uint64_t draw, float* x_prop, float* v_prop, float* p_accept, float* x_out,
                                void* ws, size_t ws_bytes, l2hmc_stream_t stream);

/* One MCMC step of the sampling loop on device-resident chains (gauge_model.py:1371-1388 around
 * apply_transition): draws (Philox streams (seed, 2*draw) for the stacked momenta [v0_f; v0_b] and
 * (seed, 2*draw+1) for coin | u -- reproducible with l2hmc_fill_normal/_uniform), both trajectories, mix,
 * accept/reject, then x <- mod(x_out, 2*pi) IN PLACE.  Per-chain outputs (any may be NULL): px = accept
 * probability; actions / plaqs / charges = observables of the step's INPUT samples (as :256-266);
 * charge_diff = |Q(x_in) - Q(x_out)| (:718-725).  ONE launch when the plan has a whole-trajectory kernel: the
 * kernel generates its own draws, a workgroup owns both directions of its chains and finishes the step in its
 * epilogue (no intermediate ever reaches HBM); other plans run the same step through the public ops.
 * draw must be below 2^63: from there on 2*draw wraps and the step would replay the streams of draw - 2^63.
 * l2hmc_gauge_mcmc_step, _ex, _ladder and l2hmc_gauge_transition_draw refuse such a draw with L2HMC_ERR_ARG (the
 * message names the entry and the value) before any device call and before the B == 0 return, as the runs do. */
size_t l2hmc_gauge_mcmc_step_ws_bytes(const l2hmc_gauge_plan* plan, int64_t B);
int l2hmc_gauge_mcmc_step(const l2hmc_gauge_plan* plan, float beta, float* x, int64_t B, uint64_t seed,
                          uint64_t draw, float* px, float* actions, float* plaqs, float* charges,
                          float* charge_diff, void* ws, size_t ws_bytes, l2hmc_stream_t stream);
/* Same step, out of place (x_next may equal x_in) and with the per-step scalars the cross-shard reduce_mean of
 * gauge_model.py:795 needs: step_sums (FOUR floats, or NULL) = [sum p_accept, sum |dQ|, B, scratch] -- the first
 * three are what a rank all-reduces per accept/reject (fixed summation order).  The fourth word is a ticket the
 * one-launch step uses to find its last workgroup: it MUST BE 0 ON ENTRY and is left at 0, so a buffer zeroed once
 * can be reused for every step. */
int l2hmc_gauge_mcmc_step_ex(const l2hmc_gauge_plan* plan, float beta, const float* x_in, float* x_next, int64_t B,
                             uint64_t seed, uint64_t draw, float* px, float* actions, float* plaqs, float* charges,
                             float* charge_diff, float* step_sums, void* ws, size_t ws_bytes,
                             l2hmc_stream_t stream);

/* l2hmc_gauge_mcmc_step_ex with a beta per chain: the rungs of a ladder -- a scan of the trained sampler over beta, or
 * the states a replica exchange (l2hmc_gauge_replica_swap) runs between -- in ONE step.  The contract of
 * l2hmc_gauge_mcmc_step_ex in every respect (the draws (seed, 2*draw) and (seed, 2*draw + 1) and their element layout,
 * the optional outputs, x_next that may alias x_in, step_sums with the ticket 0 on entry and left at 0, the workspace
 * of l2hmc_gauge_mcmc_step_ws_bytes, one launch per part of the batch on plans with a whole-step kernel, no allocation
 * and no synchronisation -- so graph capture --, B == 0 a no-op) but this: chain c runs at betas[c * chain_stride].
 * betas is a DEVICE pointer; chain_stride is 1 (betas [B]) or 0 (one value).  Both directions of a chain, the forces of
 * both momentum half-kicks of every leapfrog step and both ends of its Hamiltonian difference use the chain's value;
 * the networks never see beta.
 * The kernels run the step's own fp32 operations on the per-chain value, so chain c has the bits of
 * l2hmc_gauge_mcmc_step_ex with the same B, x_in, seed and draw at beta = betas[c * chain_stride], and step_sums is
 * the fixed-order sum of what the chains return.  Every L2HMC plan is served: plans with a whole-step kernel by an
 * instance of it that reads the chain's beta (the uniform step's kernels are left as they are), the others layer by
 * layer with the rows' betas.
 * Refused with L2HMC_ERR_ARG before any device call: NULL plan / betas / x_in / x_next, B < 0, a chain_stride other
 * than 0 or 1, hmc = 1 (l2hmc_gauge_hmc_run_ladder runs plain HMC with a beta per chain), draw >= 2^63.  A workspace that is NULL or
 * too small: L2HMC_ERR_WORKSPACE.  On plans without a whole-step kernel the plan is then checked as
 * l2hmc_gauge_transition checks it (shapes, widths, NULL masks or weights: L2HMC_ERR_ARG), also before any device call.
 * The VALUES of betas are on the device and are not checked (as in l2hmc_gauge_hmc_run_ladder): a beta that is
 * negative or not finite is no beta.  Callers check: GaugeSampler.step and GaugeSampler.run do. */
int l2hmc_gauge_mcmc_step_ladder(const l2hmc_gauge_plan* plan, const float* betas, int64_t chain_stride,
                                 const float* x_in, float* x_next, int64_t B, uint64_t seed, uint64_t draw,
                                 float* px, float* actions, float* plaqs, float* charges, float* charge_diff,
                                 float* step_sums, void* ws, size_t ws_bytes, l2hmc_stream_t stream);

/* A RUN of n_steps consecutive MCMC steps of a plain-HMC plan (plan.hmc = 1; hmc = 0 is an error), with the results
 * of n_steps calls of l2hmc_gauge_mcmc_step_ex, bit for bit.  Step s (0 <= s < n_steps) draws with index draw0 + s
 * (Philox streams (seed, 2*(draw0 + s)) and (seed, 2*(draw0 + s) + 1), the element layout of the step), runs at
 * betas[s] (a DEVICE array, so an annealed thermalisation is one call; constant beta = equal values) and starts from
 * the wrapped output of step s - 1.  Histories (each may be NULL) are [n_steps][B]: row s is what the step writes.
 * samples (or NULL) is [n_steps][B][D] and receives every step's wrapped output; the final state always goes to x_next,
 * which may alias x_in.  step_sums (or NULL) is [n_steps][4], row s = that step's [sum p_accept, sum |dQ|, B, ticket]:
 * ALL ticket words MUST BE 0 ON ENTRY and are left at 0; step_sums needs the workspace.
 * Plans for which l2hmc_gauge_plan_fused() is 1 take ONE launch: a workgroup walks its own chains through the whole
 * run with their state in registers, and every step has its own ticket and its own slice of the workspace for the
 * sums, so workgroups never wait for each other.  Other hmc plans (more than 1024 sites, L2HMC_PLAN_LAYERED) run the
 * same run as a host loop over the step; that loop reads betas back and so waits for the stream once.
 * draw0 + n_steps must not exceed 2^63 (an error otherwise): the one-launch kernel relies on bit 63 of every draw
 * index being 0.  Workspace: plans that take one launch need it only with step_sums; the host loop of the other plans
 * ALWAYS needs ws of at least l2hmc_gauge_hmc_run_ws_bytes (L2HMC_ERR_WORKSPACE otherwise), and because it
 * synchronises the stream to read betas it cannot be captured into a HIP graph (the one-launch form can).
 * n_steps <= 0 and NULL betas / x_in / x_next are errors.  l2hmc_gauge_hmc_run_ws_bytes is 0 for bad arguments and for
 * hmc = 0 (l2hmc_last_error then says so). */
size_t l2hmc_gauge_hmc_run_ws_bytes(const l2hmc_gauge_plan* plan, int64_t B, int32_t n_steps);
int l2hmc_gauge_hmc_run(const l2hmc_gauge_plan* plan, const float* betas, const float* x_in, float* x_next, int64_t B,
                        uint64_t seed, uint64_t draw0, int32_t n_steps, float* px, float* actions, float* plaqs,
                        float* charges, float* charge_diff, float* step_sums, float* samples, void* ws,
                        size_t ws_bytes, l2hmc_stream_t stream);

/* l2hmc_gauge_hmc_run with beta per step, per chain, or both, and a step size per chain: a scan over beta or over the
 * step size -- the columns of a ladder are independent runs, chains never interact -- in ONE launch.  The contract of
 * l2hmc_gauge_hmc_run in every respect (the draws (seed, 2*(draw0 + s)) and (seed, 2*(draw0 + s) + 1), the
 * [n_steps][B] histories, samples, x_next that may alias x_in, step_sums with ALL ticket words 0 on entry and left at
 * 0, the workspace only with step_sums, one launch, graph capture, draw0 + n_steps <= 2^63, B == 0 a no-op) but this:
 * step s of chain c runs at beta betas[s * step_stride + c * chain_stride], and chain c integrates with step size
 * eps_chain[c] (DEVICE pointer [B], or NULL: plan->eps for every chain).  Both directions of a chain, both of its
 * momentum half-kicks, both position sub-updates and both ends of its Hamiltonian difference use the chain's pair.
 * betas is a DEVICE pointer; a stride may be 0:
 *   (step_stride, chain_stride) = (1, 0)  a schedule, betas [n_steps]  (what l2hmc_gauge_hmc_run takes)
 *                                 (0, 1)  a ladder, betas [B]
 *                                 (B, 1)  both, betas [n_steps][B]
 *                                 (0, 0)  one value
 * The kernel runs the step's own fp32 operations on per-chain values, so column c has the bits of l2hmc_gauge_hmc_run
 * with the same B, x_in, seed and draw0 at that column's betas on a plan with eps = eps_chain[c].
 * Only plans for which l2hmc_gauge_plan_fused() is 1 are served; there is no host loop behind this entry.
 * Refused with L2HMC_ERR_ARG before any device call: NULL plan / betas / x_in / x_next, hmc = 0, a plan without the
 * one-launch kernel (more than 1024 sites, L2HMC_PLAN_LAYERED), n_steps <= 0, B < 0, a negative stride,
 * draw0 + n_steps beyond 2^63, step_sums without a workspace.  l2hmc_gauge_hmc_run_ladder_ws_bytes is
 * l2hmc_gauge_hmc_run_ws_bytes for a served plan, and 0 with l2hmc_last_error set for a plan or arguments that the
 * entry refuses.
 * The VALUES of both arrays are on the device and are not checked (as in l2hmc_small_run_tempered and
 * l2hmc_small_hmc_run): a beta that is negative or not finite is no beta, and a step size that is 0, negative or not
 * finite is no step size.  Callers check: GaugeSampler.run_hmc does. */
size_t l2hmc_gauge_hmc_run_ladder_ws_bytes(const l2hmc_gauge_plan* plan, int64_t B, int32_t n_steps);
int l2hmc_gauge_hmc_run_ladder(const l2hmc_gauge_plan* plan, const float* betas, int64_t step_stride,
                               int64_t chain_stride, const float* eps_chain, const float* x_in, float* x_next,
                               int64_t B, uint64_t seed, uint64_t draw0, int32_t n_steps, float* px, float* actions,
                               float* plaqs, float* charges, float* charge_diff, float* step_sums, float* samples,
                               void* ws, size_t ws_bytes, l2hmc_stream_t stream);

/* ONE replica-exchange (parallel tempering) round between neighbouring rungs of a beta ladder, in place on
 * x [B][2*T*X] (no plan: T, X as l2hmc_u1_plaq_sums takes them).  Columns [g * group, (g + 1) * group) form one
 * replica group and column c runs at betas[c * chain_stride] (DEVICE pointer; the stride may be 0).  A round of
 * parity 0 or 1 proposes, in every group, the disjoint pairs (a, b) = (g * group + j, g * group + j + 1) for
 * j = parity, parity + 2, ... with j + 1 < group.  Per pair: S_a, S_b = sum over plaquettes of 1 - cos P of the two
 * rows (fp32, ONE summation order, so S depends on nothing but the row);
 *   p = min(1, exp((double)(beta_a - beta_b) * ((double)S_a - (double)S_b)))   (the exponential in fp64, NaN -> 0)
 * which is exp(-beta_b S_a - beta_a S_b) / exp(-beta_a S_a - beta_b S_b); u = element a of the stream
 * l2hmc_fill_uniform(B, seed, stream_index) writes; the pair is exchanged iff p > u (strict): the two rows of x and
 * the two entries of replica trade places.  Outputs, each [B], each may be NULL: replica (int32 labels, exchanged in
 * place), action[c] = S_c for the members of a pair (other chains' entries are left untouched), swap_p[a] = p at the
 * LOWER chain of each pair and NaN elsewhere, swapped[a] = 1 / 0 at the lower chain and 0 elsewhere.
 * Any lattice size is served (up to 2^29 sites).  One launch; a round without a pair (group 2 at parity 1) fills
 * swap_p and swapped and launches nothing; B == 0 is a no-op without a device call.  Refused with L2HMC_ERR_ARG before
 * any device call: T or X <= 0, B < 0, group < 2, B not a multiple of group, parity not 0 or 1, a negative stride,
 * NULL x or betas with B > 0. */
int l2hmc_gauge_replica_swap(int32_t T, int32_t X, float* x, int64_t B, int32_t group, int32_t parity,
                             const float* betas, int64_t chain_stride, uint64_t seed, uint64_t stream_index,
                             int32_t* replica, float* action, float* swap_p, uint8_t* swapped,
                             l2hmc_stream_t stream);

/* l2hmc_gauge_hmc_run_ladder with the replica-exchange rounds of l2hmc_gauge_replica_swap INSIDE the launch: the loop
 * "run k steps, one round, run k steps, ..." of the two entries on one draw counter, bit for bit, in ONE launch.
 * The contract of l2hmc_gauge_hmc_run_ladder in every respect (optional outputs, x_next may alias x_in, step_sums with
 * ALL ticket words 0 on entry and left at 0, the workspace only with step_sums, graph capture, B == 0 a no-op), and
 * the round semantics of l2hmc_small_hmc_run_exchange: columns [g * group, (g + 1) * group) are one replica group; a
 * round runs after step s (0 <= s < n_steps) iff (swap_phase + s + 1) % swap_every == 0, on the wrapped state that step
 * left and at the betas it ran with; the j-th round of the call has parity (first_parity + j) % 2;
 * rounds = (swap_phase + n_steps) / swap_every.  swap_p (float), swapped (uint8) and replica_hist (int32), each
 * [rounds][B] and each may be NULL, receive per round what l2hmc_gauge_replica_swap writes to swap_p and swapped and
 * the labels after the round; replica (int32 [B], or NULL: the labels start as the column index) is read on entry and
 * written on exit.  samples[s] and row s of the histories are what step s wrote, BEFORE its round; x_next is the state
 * after the last round.  A round without a pair (group 2 at parity 1) fills its rows and takes its stream.
 * Streams: a step with draw index d takes (seed, 2 d) and (seed, 2 d + 1); a round after it takes the uniforms of
 * (seed, 2 d + 2), and the step after a round has draw index d + 2 (stream 2 d + 3 is skipped): what a caller gets who
 * keeps ONE counter of streams, gives a step the next even-aligned pair and a round the next stream.  So step s draws
 * with index draw0 + s + (rounds of this call before step s), and draw0 + n_steps + rounds must not exceed 2^63.
 * Served (l2hmc_gauge_hmc_run_exchange_served = 1) iff a workgroup of at most 1024 threads holds whole replica groups:
 * the plan takes l2hmc_gauge_hmc_run_ladder (hmc = 1, not layered, at most 1024 sites), its lattice has at most 512
 * sites (the instance of four sites per thread does not fit the registers of such a workgroup), and with
 *   tpc  = threads per row: the least power of two >= ceil(sites / spt), spt = 1 up to 256 sites and 2 up to 512,
 *   rpc  = rows per chain: 1 with L2HMC_PLAN_SELECTED_ONLY, else 2,
 *   cpw0 = chains per workgroup of the ladder run = (tpc == 256 ? 512 : 256) / tpc / rpc,
 * lcm(group, cpw0) * rpc * tpc <= 1024 (and the workgroup's LDS fits the 64 KiB a launch gets, which only a one-site
 * lattice with 768 rows or more can exceed).  E.g. 8x8: groups of 2, 3, 4, 6, 8 rungs (selected-only also 12 and 16); 16x16
 * and 16x32: 2 (selected-only also 4).  Every pair of rungs then meets inside one workgroup: no workgroup waits for
 * another.  The query is host logic only (no device call); it returns 0 with l2hmc_last_error set for a (plan, group)
 * that is not served, and l2hmc_gauge_replica_swap between launches of l2hmc_gauge_hmc_run_ladder takes those.
 * Refused with L2HMC_ERR_ARG before any device call: everything l2hmc_gauge_hmc_run_ladder refuses, NULL betas,
 * group < 2, B not a multiple of group, swap_every < 1, swap_phase outside [0, swap_every), first_parity not 0 or 1,
 * a (plan, group) that is not served, draw0 + n_steps + rounds beyond 2^63.  l2hmc_gauge_hmc_run_exchange_ws_bytes is
 * l2hmc_gauge_hmc_run_ladder_ws_bytes. */
int l2hmc_gauge_hmc_run_exchange_served(const l2hmc_gauge_plan* plan, int32_t group);
size_t l2hmc_gauge_hmc_run_exchange_ws_bytes(const l2hmc_gauge_plan* plan, int64_t B, int32_t n_steps);
int l2hmc_gauge_hmc_run_exchange(const l2hmc_gauge_plan* plan, const float* betas, int64_t step_stride,
                                 int64_t chain_stride, const float* eps_chain, const float* x_in, float* x_next,
                                 int64_t B, uint64_t seed, uint64_t draw0, int32_t n_steps, int32_t group,
                                 int32_t swap_every, int32_t swap_phase, int32_t first_parity, int32_t* replica,
                                 float* px, float* actions, float* plaqs, float* charges, float* charge_diff,
                                 float* step_sums, float* samples, float* swap_p, uint8_t* swapped,
                                 int32_t* replica_hist, void* ws, size_t ws_bytes, l2hmc_stream_t stream);

/* Forward value of the training loss, per chain (gauge_model.py:766-795): terms[b] = std_loss + charge_loss;
 * the scalar loss is their mean over ALL chains of all ranks.  x, x_prop, z: [B][2*T*X]; px, pz: [B].
 * metric: 0 'l1', 1 'l2', 2 'cos', 3 'cos2', 4 'cos_diff' (:632-657).  Both auxiliary terms compare z with
 * x_prop, exactly as the reference writes them. */
int l2hmc_gauge_loss_terms(const float* x, const float* x_prop, const float* px, const float* z,
                           const float* pz, int64_t B, int32_t T, int32_t X, int32_t metric,
                           float loss_scale, float aux_weight, float std_weight, float charge_weight,
                           float* terms, l2hmc_stream_t stream);

/* ------------------------------------------------------------------------
 * Training: gradients of the loss with respect to the network weights and the step size, and the
 * optimiser step -- tf.gradients(loss, dynamics.variables) + AdamOptimizer.apply_gradients of
 * gauge_model.py:799-830, :942-969.  GenericNet and ConvNet3D plans (hmc = 0).
 *
 * Chains are integrated in the direction their coin selects (rows = x chains then z chains for the
 * loss of gauge_model.py:728-797; the masked-out direction carries exactly zero gradient in the
 * reference's graph).  The sequence for one training step is
 *   l2hmc_gauge_train_forward   -> x_N, v_N, sumlogdet, p        (keeps every intermediate in `ws`)
 *   l2hmc_gauge_loss_backward   -> per-chain loss, d loss / d (x_N, v_N, sumlogdet)
 *   l2hmc_gauge_train_backward  -> gradients (same k-contiguous layout as struct l2hmc_dense_net)
 *   [all-reduce of the flat gradient buffers across ranks]
 *   l2hmc_grad_sumsq / l2hmc_adam_step
 * ------------------------------------------------------------------------ */
typedef struct l2hmc_dense_grads {
  float* w1_t;     /* [H][Ka+Kb] */
  float* wt;       /* [2][H]  */
  float* b1;       /* [H]: gradient of EACH of the three first-layer biases (they are summed in b1) */
  float* wh_t;     /* [H][H]  */
  float* bh;       /* [H]     */
  float* whd_t;    /* [3][D][H] */
  float* bhd;      /* [3][D]  */
  float* coeff_s;  /* [D]     */
  float* coeff_q;  /* [D]     */
} l2hmc_dense_grads;

/* Gradients of a ConvNet3D front-end, in the Keras layout of the weights (struct l2hmc_conv3d_front);
 * the dd = 1 slice of the second kernel only ever multiplies padding, so its gradient is exactly 0. */
typedef struct l2hmc_conv3d_grads {
  float* w1_a; float* b1_a; float* w2_a; float* b2_a;   /* first input  */
  float* w1_b; float* b1_b; float* w2_b; float* b2_b;   /* second input */
} l2hmc_conv3d_grads;

/* Bytes of the tape and scratch of one training step over `rows` rows (0 for hmc = 1).  A plan with
 * L2HMC_PLAN_PERIODIC | L2HMC_PLAN_PERIODIC_TRAIN tapes a first-layer input of 3D columns per network call instead of
 * 2D and carries a [rows][3D] input cotangent instead of [rows][2D]; against the same plan without
 * L2HMC_PLAN_PERIODIC_TRAIN it takes, with N = num_steps and D = 2*T*X (a multiple of 32),
 *   2 * (2 N * rows * D * 4)  +  round_up(rows * 3 D * 4, 256) - rows * 2 D * 4   bytes more
 * (both networks' input tapes, and the input cotangent rounded to the 256-byte grid every section starts on).  No other
 * plan's size depends on the flag. */
size_t l2hmc_gauge_train_ws_bytes(const l2hmc_gauge_plan* plan, int64_t rows);
/* How l2hmc_gauge_train_forward[_ladder] runs a plan (host logic only, no device call, no reference counterpart):
 * 1 = as ONE launch of a taped whole-trajectory kernel -- the reference-mode plans with such a kernel (GenericNet on
 * D = 128, ConvNet3D on 8x8) and the torus-exact plans L2HMC_PLAN_PERIODIC_TAPE describes; 0 = layer by layer (also with
 * L2HMC_PLAN_LAYERED); negative = a plan the training entries refuse (l2hmc_last_error says why). */
int l2hmc_gauge_plan_train_fused(const l2hmc_gauge_plan* plan);
/* Same outputs as l2hmc_gauge_trajectory (dir: per-row 0 forward / 1 backward, NULL = all forward);
 * `ws` must stay untouched until the matching l2hmc_gauge_train_backward has run. */
int l2hmc_gauge_train_forward(const l2hmc_gauge_plan* plan, float beta, const float* x0, const float* v0,
                              const int32_t* dir, int64_t rows, float* x_out, float* v_out, float* sumlogdet,
                              float* p_accept, void* ws, size_t ws_bytes, l2hmc_stream_t stream);
/* dx, dv: [rows][D] = d loss / d (x_N, v_N) on entry, overwritten (d loss / d (x_0, v_0) on exit);
 * dlogdet: [rows] = d loss / d sumlogdet.  gx, gv, deps (1 float) are overwritten with the gradients.
 * gxf, gvf: for L2HMC_PLAN_CONV3D plans, where the gradients of the Conv3D kernels / biases go; NULL for
 * GenericNet plans. */
int l2hmc_gauge_train_backward(const l2hmc_gauge_plan* plan, float beta, const int32_t* dir, int64_t rows,
                               float* dx, float* dv, const float* dlogdet, const l2hmc_dense_grads* gx,
                               const l2hmc_dense_grads* gv, const l2hmc_conv3d_grads* gxf,
                               const l2hmc_conv3d_grads* gvf, float* deps, void* ws, size_t ws_bytes,
                               l2hmc_stream_t stream);
/* The same pass with BUCKET NOTIFICATIONS for a data-parallel caller (gauge_model.py:942-943: Horovod's
 * DistributedOptimizer all-reduces gradients tensor by tensor while the rest of the backward graph still runs).
 * The weight gradients are finished in seven contiguous groups; as soon as everything that produces group b has
 * been ENQUEUED on `stream`, `on_bucket(user, b)` runs on the calling host thread -- the caller records an event
 * there and starts its collective for that group on another stream, so the exchange of group b overlaps the
 * computation of group b + 1.  Groups, in the order they complete (k = 0: gx, k = 1: gv):
 *   3k + 0: w1_t, wt, b1        3k + 1: wh_t, bh        3k + 2: whd_t, bhd, coeff_s, coeff_q
 *   L2HMC_GRAD_BUCKET_REST (6): Conv3D front-end gradients (gxf, gvf) and deps -- always last.
 * Results are identical to l2hmc_gauge_train_backward. */
#define L2HMC_GRAD_BUCKET_REST 6
typedef void (*l2hmc_bucket_fn)(void* user, int32_t bucket);
int l2hmc_gauge_train_backward_buckets(const l2hmc_gauge_plan* plan, float beta, const int32_t* dir, int64_t rows,
                                       float* dx, float* dv, const float* dlogdet, const l2hmc_dense_grads* gx,
                                       const l2hmc_dense_grads* gv, const l2hmc_conv3d_grads* gxf,
                                       const l2hmc_conv3d_grads* gvf, float* deps, void* ws, size_t ws_bytes,
                                       l2hmc_stream_t stream, l2hmc_bucket_fn on_bucket, void* user);
/* Loss (gauge_model.py:728-797) and its gradient with respect to the proposed states of the 2B stacked
 * chains (rows [0,B): started at x; rows [B,2B): started at z), through the accept probabilities
 * (gauge_dynamics.py:592-609).  x0, xN, vN: [2B][2*T*X]; p: [2B]; inv_count = 1 / (number of chains the
 * mean of :795 runs over, all ranks); terms: [B] or NULL; dxN, dvN: [2B][D]; dlogdet: [2B]. */
int l2hmc_gauge_loss_backward(int32_t T, int32_t X, float beta, const float* x0, const float* xN,
                              const float* vN, const float* p, int64_t B, int32_t metric, float loss_scale,
                              float aux_weight, float std_weight, float charge_weight, float inv_count,
                              float* terms, float* dxN, float* dvN, float* dlogdet, l2hmc_stream_t stream);
/* The training step on a LADDER of beta: the three entries above with a beta per chain, for networks that are to
 * serve every rung of a replica-exchange run (l2hmc_gauge_mcmc_step_ladder, l2hmc_gauge_replica_swap).  Row r of a
 * call reads betas[(r % chains) * chain_stride]: with chains = B, rows i and B + i of the stacked 2B rows (chain i of
 * the x batch and chain i of the z batch) train at one value.  betas is a DEVICE pointer; chain_stride is 1 (betas
 * [chains]) or 0 (one value).  Everything else is the contract of the scalar entry: arguments, outputs, the workspace
 * of l2hmc_gauge_train_ws_bytes, no allocation, rows == 0 / B == 0 a no-op -- with ONE exception:
 * l2hmc_gauge_train_backward_ladder takes rows == 0 as a no-op too (plan and ladder arguments are still checked, nothing
 * is written), where the two scalar backward entries refuse it.  The kernels run the scalar step's own
 * fp32 operations on the row's value, so a row has the bits of the scalar entry at its beta (weight and eps gradients
 * are sums over rows and have them where all rows share one value).  Every training plan is served: plans with a
 * whole-trajectory kernel by instances of it, and of the fused reverse pass, that read the row's beta from LDS (the
 * uniform entries' kernels are left as they are), the others layer by layer with the rows' betas.
 * l2hmc_gauge_train_backward_ladder covers both scalar backward entries: on_bucket may be NULL.
 * l2hmc_gauge_loss_backward_ladder lays the ladder on the B pairs: rows r and B + r read betas[r * chain_stride].
 * Refused with L2HMC_ERR_ARG before any device call: NULL betas, a chain_stride other than 0 or 1, chains <= 0,
 * rows % chains != 0, and everything the scalar entry refuses.
 * The VALUES of betas are on the device and are not checked (as in l2hmc_gauge_mcmc_step_ladder): a beta that is
 * negative or not finite is no beta.  Callers check: GaugeTrainer.calc_loss_and_grads does. */
int l2hmc_gauge_train_forward_ladder(const l2hmc_gauge_plan* plan, const float* betas, int64_t chain_stride,
                                     int64_t chains, const float* x0, const float* v0, const int32_t* dir,
                                     int64_t rows, float* x_out, float* v_out, float* sumlogdet, float* p_accept,
                                     void* ws, size_t ws_bytes, l2hmc_stream_t stream);
int l2hmc_gauge_train_backward_ladder(const l2hmc_gauge_plan* plan, const float* betas, int64_t chain_stride,
                                      int64_t chains, const int32_t* dir, int64_t rows, float* dx, float* dv,
                                      const float* dlogdet, const l2hmc_dense_grads* gx, const l2hmc_dense_grads* gv,
                                      const l2hmc_conv3d_grads* gxf, const l2hmc_conv3d_grads* gvf, float* deps,
                                      void* ws, size_t ws_bytes, l2hmc_stream_t stream, l2hmc_bucket_fn on_bucket,
                                      void* user);
int l2hmc_gauge_loss_backward_ladder(int32_t T, int32_t X, const float* betas, int64_t chain_stride, const float* x0,
                                     const float* xN, const float* vN, const float* p, int64_t B, int32_t metric,
                                     float loss_scale, float aux_weight, float std_weight, float charge_weight,
                                     float inv_count, float* terms, float* dxN, float* dvN, float* dlogdet,
                                     l2hmc_stream_t stream);
/* Reverse of the end of a transition (gauge_dynamics.py:229-257) for ANY loss: the accept probability
 * p = exp(min(A, 0)), A = H(x0, v0) - H(xN, vN) + sumlogdet, H = beta S(x) + |v|^2 / 2, and the select
 * x_out = a xN + (1 - a) x0 with a = [p > u] (strict).  What a caller's autograd needs between its cotangents of
 * (x_prop, v_prop, p, x_out) and l2hmc_gauge_train_backward.  With g = g_p p where 0 < p < 1 (else 0) and
 * F = beta dS/dx (the `force` of l2hmc_u1_action_force):
 *   dxN = g_xprop + a g_xout - g F(xN)      dvN = g_vprop - g vN      dlogdet = g
 *   dx0 = (1 - a) g_xout + g F(x0)          dv0 = g v0
 * dx0 / dv0 are only the DIRECT dependence on the start state; l2hmc_gauge_train_backward adds the part through
 * the trajectory.  x0, v0, xN, vN, dxN, dvN, dx0, dv0: [rows][2*T*X]; p, u, g_p, dlogdet: [rows].  Each g_* may be
 * NULL (= 0); dx0, dv0 may be NULL (not written; v0 may then be NULL).  Rows with g = 0 never form 0 * F, so a
 * non-finite proposal (p = 0) leaves the other terms finite.  One wave per row, the chain staged in LDS. */
int l2hmc_gauge_accept_backward(int32_t T, int32_t X, float beta, int64_t rows, const float* x0, const float* v0,
                                const float* xN, const float* vN, const float* p, const float* u,
                                const float* g_xprop, const float* g_vprop, const float* g_p, const float* g_xout,
                                float* dxN, float* dvN, float* dlogdet, float* dx0, float* dv0,
                                l2hmc_stream_t stream);
/* l2hmc_gauge_accept_backward with a beta per row: F = beta_r dS/dx in the dxN and dx0 terms, beta_r =
 * betas[(r % chains) * chain_stride] (betas a DEVICE pointer, chain_stride 1 or 0: the convention of
 * l2hmc_gauge_train_forward_ladder, between whose forward and l2hmc_gauge_train_backward_ladder it stands).  An
 * instance of the same kernel: a row has the bits of the scalar entry at its beta, a row with g = 0 still never forms
 * 0 * F (and does not read its beta), the LDS bound and the lattices served are the scalar entry's.  rows == 0 is a
 * no-op after the checks.  Refused with L2HMC_ERR_ARG before any device call: NULL betas, a chain_stride other than 0
 * or 1, chains <= 0, rows % chains != 0, and everything the scalar entry refuses.  The VALUES of betas are not
 * checked. */
int l2hmc_gauge_accept_backward_ladder(int32_t T, int32_t X, const float* betas, int64_t chain_stride, int64_t chains,
                                       int64_t rows, const float* x0, const float* v0, const float* xN,
                                       const float* vN, const float* p, const float* u, const float* g_xprop,
                                       const float* g_vprop, const float* g_p, const float* g_xout, float* dxN,
                                       float* dvN, float* dlogdet, float* dx0, float* dv0, l2hmc_stream_t stream);
/* *out (device) = [*out +] sum g[i]^2, elements in [tri_lo, tri_hi) counted three times (the packed
 * first-layer bias stands for three reference variables); fixed summation order. */
int l2hmc_grad_sumsq(const float* g, int64_t n, int64_t tri_lo, int64_t tri_hi, float* out, int32_t accumulate,
                     l2hmc_stream_t stream);
/* Adam as tf.train.AdamOptimizer applies it: m, v moments; lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t) is
 * computed by the caller; w -= lr_t * m / (sqrt(v) + eps).  gnorm_sq (device scalar) != NULL applies
 * tf.clip_by_global_norm(clip) first.  Elements in [tri_lo, tri_hi) move three times as far (see above). */
int l2hmc_adam_step(float* w, const float* g, float* m, float* v, int64_t n, float lr_t, float beta1,
                    float beta2, float eps, const float* gnorm_sq, float clip, int64_t tri_lo, int64_t tri_hi,
                    l2hmc_stream_t stream);

/* ------------------------------------------------------------------------
 * Generic integrator on 2-D toy targets (MoG / SCG):
 *   utils/dynamics.py:120-225,255-319; utils/sampler.py:28-59;
 *   utils/distributions.py:32-39,63-68,151-158 (mixture, Gaussian), :101-121 (rough well), :184-211 (funnel).
 * Target kinds (l2hmc_mog_target::is_gaussian holds the kind; 0 and 1 mean what they always did):
 *   L2HMC_TARGET_MIXTURE     mixture of K Gaussians:
 *       energy(x) = -logsumexp_k( -0.5 (x-mu_k)^T P_k (x-mu_k) + log_const[k] )
 *   L2HMC_TARGET_GAUSSIAN    K = 1, log_const ignored: energy(x) = 0.5 (x-mu)^T P (x-mu)
 *   L2HMC_TARGET_ROUGH_WELL  energy(x) = 0.5 sum_i x_i^2 + eps sum_i cos(x_i / a), a = eps^2, or a = eps when `easy`;
 *       x_i / a is a division by the fp32 product eps * eps (the reference's operation order)
 *   L2HMC_TARGET_FUNNEL      v = x_0, n = dim - 1, s = exp(v):
 *       energy(x) = 0.5 (v^2 / 4 + sum_{i>=1} x_i^2 / s + n log(2 pi s)),
 *       with s the constant exp(8) where v > 8 and exp(-8) where v < -8 (strict comparisons: v = +-8 is unclipped);
 *       gradient and Hessian follow the selected branch, as tf.gradients of tf.where does.  sigma = 2 and the clip
 *       4 sigma = 8 are the reference's constants (its constructor ignores its `clip` argument).  dim >= 2.
 * Every kind's energy, gradient and Hessian are divided by `temperature`.
 * The two analytic kinds take no device memory: K = 1, prec and log_const are ignored (may be NULL), and the rough
 * well's two scalars travel by value in the slot of `mu` (same size and offset: the layout and L2HMC_ABI_VERSION are
 * unchanged).  An unknown kind, a funnel with dim < 2 and a rough well with eps <= 0 (or not finite) are refused with
 * L2HMC_ERR_ARG before any launch by every entry that takes a target or a plan.
 * ------------------------------------------------------------------------ */
/* Limits of this path (utils/network.py:89-114 takes any x_dim / num_nodes; the reference's own configurations are
 * 2-D targets with num_nodes 10 (SCGExperiment.ipynb) and 50 (mog_model.py, network.py:89)): x_dim <= 8 for every
 * target kind, with at most 8 mixture components (the closed-form energy, its gradient and Hessian-vector product
 * live in registers; the rough well and the funnel have no parameter arrays at all), and num_nodes <= 64 (both
 * networks' weights stay in LDS for the whole trajectory).  Larger values are refused with L2HMC_ERR_ARG; wider toy
 * networks, higher dimensions and any other energy belong on the layer-by-layer path above. */
#define L2HMC_MAX_MIX 8
#define L2HMC_MAX_SMALL_DIM 8
#define L2HMC_TARGET_MIXTURE 0
#define L2HMC_TARGET_GAUSSIAN 1
#define L2HMC_TARGET_ROUGH_WELL 2
#define L2HMC_TARGET_FUNNEL 3
typedef struct l2hmc_mog_target {
  int32_t dim;                     /* <= L2HMC_MAX_SMALL_DIM */
  int32_t K;                       /* <= L2HMC_MAX_MIX; 1 for every kind but the mixture */
  int32_t is_gaussian;             /* the kind: one of L2HMC_TARGET_* (1: energy = 0.5 (x-mu)^T P (x-mu)) */
  float temperature;
  union {
    const float* mu;               /* mixture, Gaussian: [K][dim] */
    struct {
      float eps;                   /* rough well: > 0 */
      int32_t easy;                /* rough well: 0: a = eps^2; otherwise a = eps */
    } rough_well;
  };
  const float* prec;               /* mixture, Gaussian: [K][dim][dim] inverse covariances */
  const float* log_const;          /* mixture: [K] log(pi_k / sqrt((2pi)^dim det Sigma_k)) */
} l2hmc_mog_target;

typedef struct l2hmc_small_plan {
  int32_t x_dim, num_nodes, trajectory_length, hmc;
  float eps;
  int32_t first_layer_form;        /* 0: chosen by batch size; 1 / 2: force the matrix-pipe / VALU form of the first layer;
                                    * 3: two waves per group of 16 rows (latency form, 17..64 hidden units).  The forms
                                    * group their sums differently and agree to rounding */
  const float* masks;              /* [trajectory_length][x_dim] */
  l2hmc_dense_net xnet, vnet;      /* q_tanh = 1, Ka = Kb = x_dim */
  l2hmc_mog_target target;
} l2hmc_small_plan;

int l2hmc_mog_energy_grad(const l2hmc_mog_target* tgt, const float* x, int64_t rows, float* energy,
                          float* grad, l2hmc_stream_t stream);

/* Dynamics.forward / .backward (dir per row, NULL = all forward): whole
 * trajectory per chain in one kernel. */
int l2hmc_small_trajectory(const l2hmc_small_plan* plan, const float* x0, const float* v0,
                           const int32_t* dir, int64_t rows, float* x_out, float* v_out,
                           float* sumlogdet, float* p_accept, l2hmc_stream_t stream);
/* l2hmc_small_trajectory on a LADDER of temperatures: row r runs at temps[(r % chains) * chain_stride], temps a DEVICE
 * array, chain_stride 1 (temps [chains]) or 0 (one value) -- the convention of l2hmc_small_train_step_tempered.  With
 * both directions of B chains stacked (rows = 2 B, chains = B) rows i and B + i share temps[i].
 * plan->target.temperature is IGNORED (it must still be > 0).  Every plan l2hmc_small_trajectory serves is served: all
 * four target kinds, every first_layer_form, hmc plans; the form is chosen by the rows as there.  The row's 1 / t is
 * formed once, by the division the other instances use: a row has the bits of l2hmc_small_trajectory on a plan at its
 * temperature.  rows == 0 is a no-op after the checks.  Refused with L2HMC_ERR_ARG before any launch: NULL temps, a
 * chain_stride other than 0 or 1, chains <= 0, rows % chains != 0, and everything l2hmc_small_trajectory refuses.  The
 * VALUES of temps are not checked here (Dynamics / propose check them: finite and > 0 in float32). */
int l2hmc_small_trajectory_tempered(const l2hmc_small_plan* plan, const float* temps, int64_t chain_stride,
                                    int64_t chains, const float* x0, const float* v0, const int32_t* dir,
                                    int64_t rows, float* x_out, float* v_out, float* sumlogdet, float* p_accept,
                                    l2hmc_stream_t stream);

/* utils/sampler.py:28-55 `propose` (and :57-59 `tf_accept` when x_out != NULL) in ONE launch for the L2HMC sampler
 * (plan->hmc == 0).  Chain c's direction bit, forward momentum, backward momentum and Metropolis-Hastings uniform are
 * the Philox streams (seed, draw0), (seed, draw0 + 1), (seed, draw0 + 2), (seed, draw0 + 3): exactly the elements
 * l2hmc_fill_uniform(B) / l2hmc_fill_normal(B * x_dim) write with those (seed, offset) pairs, so the call equals
 * fill x 4 + l2hmc_small_trajectory(2B rows) + l2hmc_mix_accept(strict = 0) bit for bit.  Both trajectories of a
 * chain run in the same wave.  Outputs (each may be NULL): Lx, Lv [B][x_dim] the proposal selected by the direction
 * bit (forward iff uniform >= 0.5), px [B] its accept probability, x_out [B][x_dim] = Lx where px - u >= 0 else x.
 * draw0 must not exceed 2^64 - 4: beyond it the last of the four streams would wrap onto streams 0, 1, 2.  Refused
 * with L2HMC_ERR_ARG (the message gives the value) before any device call and before the B == 0 return. */
int l2hmc_small_propose(const l2hmc_small_plan* plan, const float* x, int64_t B, uint64_t seed, uint64_t draw0,
                        float* Lx, float* Lv, float* px, float* x_out, l2hmc_stream_t stream);

/* A RUN of n_steps consecutive sampler steps of an L2HMC plan (plan->hmc == 0; hmc != 0 is refused as by
 * l2hmc_small_propose), with the results of n_steps calls of l2hmc_small_propose(plan, x, B, seed, draw0 + 4 s, NULL,
 * NULL, px + s B, x_out) chained through x_out, bit for bit.  Step s (0 <= s < n_steps) takes its direction bits,
 * forward momenta, backward momenta and Metropolis-Hastings uniforms from the Philox streams (seed, draw0 + 4 s) ..
 * (seed, draw0 + 4 s + 3) and starts from the output of step s - 1 (step 0 from x_in).  px (or NULL) is [n_steps][B]:
 * row s holds the step's accept probabilities.  samples (or NULL) is [n_steps][B][x_dim] and receives every step's
 * output; the final state always goes to x_next [B][x_dim], which may alias x_in.
 * ONE launch, of the kernel and in the form l2hmc_small_propose takes for the same B: a wave keeps both directions of
 * its eight chains in registers from step to step and stages the weights, the target, the masks and the time table
 * once.  Waves never wait for each other, so there is no workspace, no ticket and no host synchronisation, and the call
 * can be captured into a HIP graph.
 * draw0 + 4 n_steps must not exceed 2^64 - 1 (an error otherwise).  n_steps <= 0 and NULL plan / x_in / x_next are
 * errors, as is everything l2hmc_small_propose refuses; all are reported before any device call.  B == 0 is a no-op. */
int l2hmc_small_run(const l2hmc_small_plan* plan, const float* x_in, float* x_next, int64_t B, uint64_t seed,
                    uint64_t draw0, int32_t n_steps, float* px, float* samples, l2hmc_stream_t stream);

/* l2hmc_small_run with a temperature per step, per chain, or both: an annealed burn-in or a ladder of temperatures in
 * ONE launch.  The contract of l2hmc_small_run in every respect (the draws (seed, draw0 + 4 s .. + 3), px, samples,
 * x_next that may alias x_in, one launch, no workspace, graph capture, B == 0 a no-op) but one: step s of chain c runs
 * at temperature temps[s * step_stride + c * chain_stride], both of its directions and both ends of its Hamiltonian
 * difference alike.  temps is a DEVICE pointer; a stride may be 0:
 *   (step_stride, chain_stride) = (1, 0)  a schedule, temps [n_steps]
 *                                 (0, 1)  a ladder, temps [B]
 *                                 (B, 1)  both, temps [n_steps][B]
 * plan->target.temperature is not used (it must still be > 0, as everywhere).  The kernel forms 1 / t as the other
 * entries form 1 / temperature, so a run whose entries all equal T gives the bits of l2hmc_small_run on a plan with
 * temperature = T.
 * Refused with L2HMC_ERR_ARG before any device call: everything l2hmc_small_run refuses, NULL temps, a negative stride.
 * The VALUES are on the device and are not checked.  An entry of 0 or NaN gives its chain a non-finite energy and
 * gradient in that step, which by the rule of every entry here is an accept probability of 0 -- the chain stays where
 * it is.  A negative entry is not refused either and is no temperature (finite energies of the wrong sign: the step
 * targets exp(+E / |t|)), and +infinity is the flat target.  Callers that cannot vouch for their temperatures check
 * them first: finite and > 0 (DynamicsSampler.run does). */
int l2hmc_small_run_tempered(const l2hmc_small_plan* plan, const float* x_in, float* x_next, int64_t B,
                             uint64_t seed, uint64_t draw0, int32_t n_steps,
                             const float* temps, int64_t step_stride, int64_t chain_stride,
                             float* px, float* samples, l2hmc_stream_t stream);

/* A RUN of n_steps consecutive sampler steps of a plain-HMC plan (plan->hmc != 0: no networks, the forward trajectory
 * only, utils/sampler.py:30-32) in ONE launch, with the results of the loop over l2hmc_fill_normal(seed, draw0 + 2 s),
 * l2hmc_small_trajectory, l2hmc_fill_uniform(seed, draw0 + 2 s + 1) and l2hmc_mix_accept(strict = 0, coin = 1, the
 * proposal in both slots) chained through its output, bit for bit.  Step s takes its momenta (element c * x_dim + d for
 * chain c) and its Metropolis-Hastings uniforms (element c) from those two Philox streams and starts from the output
 * of step s - 1 (step 0 from x_in).  px (or NULL) is [n_steps][B], samples (or NULL) [n_steps][B][x_dim] with every
 * step's output; the final state always goes to x_next [B][x_dim], which may alias x_in.
 * A kernel of its own (small_hmc.hip): one thread per chain with the chain in registers for the whole launch, one wave
 * per workgroup, the target and the masks staged once.  No workspace, no host synchronisation; the call can be captured
 * into a HIP graph.  plan->xnet / vnet / num_nodes / first_layer_form are not read.
 * temps (DEVICE pointer, or NULL: plan->target.temperature for every step and chain) has the meaning and the strides
 * of l2hmc_small_run_tempered: step s of chain c runs at temps[s * step_stride + c * chain_stride]; the strides are
 * not read when temps is NULL.  eps_chain (DEVICE pointer, or NULL: plan->eps for every chain) is [B]: chain c
 * integrates with step size eps_chain[c].  Chains never interact, so the columns of a ladder of temperatures or of
 * step sizes are independent runs.  The VALUES of both arrays are not checked (as in l2hmc_small_run_tempered; a step
 * size that is 0, negative or not finite is no step size: callers check, DynamicsSampler.run_hmc does).
 * Refused with L2HMC_ERR_ARG before any device call: NULL plan / x_in / x_next, B < 0, n_steps <= 0, an L2HMC plan
 * (hmc == 0: that is l2hmc_small_run's), draw0 + 2 n_steps beyond 2^64 - 1, a negative stride, x_dim != target.dim,
 * trajectory_length <= 0 or NULL masks (or more masks than 64 KiB of LDS hold), and what every entry refuses of a
 * target.  B == 0 is a no-op. */
int l2hmc_small_hmc_run(const l2hmc_small_plan* plan, const float* x_in, float* x_next, int64_t B, uint64_t seed,
                        uint64_t draw0, int32_t n_steps, const float* temps, int64_t step_stride, int64_t chain_stride,
                        const float* eps_chain, float* px, float* samples, l2hmc_stream_t stream);

/* Annealed importance sampling (utils/ais.py:30-82, after Wu et al. 2016) on a packed toy target: a RUN of n_steps
 * annealing steps in ONE launch.  E1 is the plan target's energy at the plan's temperature -- exactly what
 * l2hmc_small_hmc_run integrates; every kind, x_dim <= 8 -- and E0 the energy of `init`, a target of kind
 * L2HMC_TARGET_GAUSSIAN and the plan's dim, evaluated at temperature 1 whatever its field says.  The launch estimates
 * log(Z1 / Z0), Z = integral of exp(-E): the mean over chains of exp(log_w), taken by the caller.
 * betas is a DEVICE float[n_steps + 1]: step s of the launch (0 <= s < n_steps) reads betas[s] as b_{s-1} and
 * betas[s + 1] as b_s, so a run cut into launches passes the same array at an offset.  Per chain, step s does
 *   log_w += ((double)b_s - (double)b_{s-1}) * ((double)E0(x) - (double)E1(x))   on the state step s - 1 left (:56-57)
 *   momentum: fresh N(0, I) (:55); with v given, v * sqrt(1 - refreshment) + n * sqrt(refreshment), n ~ N(0, I) (:53)
 *   one forward plain-HMC trajectory (the plan's masks, eps, trajectory_length) on E_s = (1.f - b_s) * E0 + b_s * E1,
 *   formed in float32 like that, the gradient likewise: at b_s = 1 the step has the bits of l2hmc_small_hmc_run on the
 *   plan, at b_s = 0 those of a run on a plan whose target is `init` at temperature 1
 *   p = exp(min(0, H_s(x, v) - H_s(Lx, Lv))), a non-finite value gives 0; accepted iff p - u >= 0 (:61)
 *   accepted: x <- Lx, v <- Lv; rejected: x stays, v <- -Lv -- the PROPOSED momentum negated (:63), not the one the step
 *   started from
 * Draws: two streams per step in the layout of l2hmc_small_hmc_run: the momenta, or the noise n, are elements
 * c * x_dim + d of stream (seed, draw0 + 2 s), the Metropolis-Hastings uniform is element c of (seed, draw0 + 2 s + 1).
 * log_w is a DEVICE double[B], read and written (a fresh anneal starts it at 0); the increment and the sum are formed in
 * double, so a run cut into launches has the bits of the uncut one.  v is a DEVICE float[B][x_dim], read and written,
 * or NULL: fresh momenta every step, and refreshment is not read.  px (or NULL) is [n_steps][B].  The final state goes
 * to x_next [B][x_dim], which may alias x_in.
 * A kernel of its own (small_ais.hip) in the geometry of l2hmc_small_hmc_run: one thread per chain with x, v, the
 * gradient and log_w in registers for the whole launch, one wave per workgroup, both targets and the masks staged once.
 * No workspace, no host synchronisation; the call can be captured into a HIP graph.  The VALUES of betas are not
 * checked (callers check: finite, in [0, 1], non-decreasing; DynamicsSampler.ais does).
 * Refused with L2HMC_ERR_ARG before any device call: NULL plan / init / x_in / x_next / betas / log_w, B < 0,
 * n_steps <= 0, an L2HMC plan (hmc == 0), what l2hmc_small_hmc_run refuses of a plan and its target, an init of another
 * kind or dim (or with NULL mu / prec), refreshment outside (0, 1] when v is given, draw0 + 2 n_steps beyond 2^64 - 1,
 * targets and masks beyond 64 KiB of LDS.  B == 0 is a no-op. */
int l2hmc_small_ais_run(const l2hmc_small_plan* plan, const l2hmc_mog_target* init, const float* x_in, float* x_next,
                        float* v, float refreshment, int64_t B, uint64_t seed, uint64_t draw0, int32_t n_steps,
                        const float* betas, double* log_w, float* px, l2hmc_stream_t stream);

/* ONE replica-exchange (parallel tempering) round between neighbouring rungs of a temperature ladder on a packed toy
 * target, in place on x [B][x_dim].  Any plan with a packed target is served, an L2HMC sampler's included: of the plan
 * only x_dim and target are read.  Columns [g * group, (g + 1) * group) form one replica group and column c is at
 * temperature temps[c * chain_stride] (DEVICE pointer; the stride may be 0; the values are not checked, as in
 * l2hmc_small_run_tempered).  A round of parity 0 or 1 proposes, in every group, the disjoint pairs
 * (a, b) = (g * group + j, g * group + j + 1) for j = parity, parity + 2, ... with j + 1 < group, the rule of
 * l2hmc_gauge_replica_swap.  Per pair: U_a, U_b = the target's energy at temperature 1 of the two rows (fp32, the
 * arithmetic of l2hmc_mog_energy_grad: U depends on nothing but the row and the target), it = 1.f / temperature as
 * every step forms it;
 *   p = min(1, exp(((double)it_a - (double)it_b) * ((double)U_a - (double)U_b)))   (the exponential in fp64, NaN -> 0)
 * which is exp(-U_b / T_a - U_a / T_b) / exp(-U_a / T_a - U_b / T_b); u = element a of the stream
 * l2hmc_fill_uniform(B, seed, stream_index) writes; the pair is exchanged iff p > u (strict): the two rows of x and
 * the two entries of replica trade places, temperatures stay with the column.  Outputs, each [B], each may be NULL:
 * replica (int32 labels, exchanged in place), energy[c] = U_c for the members of a pair (other chains' entries are
 * left untouched), swap_p[a] = p at the LOWER chain of each pair and NaN elsewhere, swapped[a] = 1 / 0 at the lower
 * chain and 0 elsewhere (the chains that sit the round out included).
 * One thread per chain, a group inside one wave (hence group <= 64).  One launch (profile class 8); a round without a
 * pair (group 2 at parity 1) fills swap_p and swapped and launches nothing; B == 0 is a no-op.  Refused with
 * L2HMC_ERR_ARG before any device call: NULL plan, B < 0, group < 2 or > 64, B not a multiple of group, parity not 0
 * or 1, a negative stride, x_dim != target.dim and what every entry refuses of a target, NULL x or temps with B > 0. */
int l2hmc_small_replica_swap(const l2hmc_small_plan* plan, float* x, int64_t B, int32_t group, int32_t parity,
                             const float* temps, int64_t chain_stride, uint64_t seed, uint64_t stream_index,
                             int32_t* replica, float* energy, float* swap_p, uint8_t* swapped,
                             l2hmc_stream_t stream);

/* l2hmc_small_hmc_run with replica exchange between the columns of a temperature ladder INSIDE the launch: its contract
 * (momenta and Metropolis-Hastings uniforms per step, px, samples, x_next that may alias x_in, temps with its strides,
 * eps_chain, no workspace, graph capture, the same bits on every run, B == 0 a no-op) with these differences.
 * After step s of the launch one round of l2hmc_small_replica_swap (group, the rule and the arithmetic above) runs iff
 * (swap_phase + s + 1) % swap_every == 0, on the state the step left and at the temperatures the step ran with
 * (temps[s * step_stride + c * chain_stride]); the j-th round of the launch has parity (first_parity + j) % 2.
 * Streams are taken in the order of the loop a caller would write: a step takes two (momenta, uniforms), a round the
 * next one -- a round without a pair takes its stream as well, so the accounting does not depend on the group size.
 * The launch consumes streams draw0 .. draw0 + 2 n_steps + rounds - 1, rounds = (swap_phase + n_steps) / swap_every.
 * samples[s] and px[s] are step s's own outputs, taken BEFORE its round; the round shows in the next step's input and
 * in x_next.  replica [B] (int32 labels, or NULL) is read on entry and written on exit.  swap_p, swapped and
 * replica_hist (the labels after each round) are [rounds][B]; each may be NULL.
 * ONE launch (profile class 7) of the run kernel: a workgroup (one wave) holds (64 / group) * group chains, so a group
 * never straddles a wave and a round is a handful of cross-lane reads between two steps.  Bit for bit the loop
 * l2hmc_small_hmc_run (up to the next round), l2hmc_small_replica_swap: both call one device function on the fp32
 * state the run would store and reload.
 * Refused with L2HMC_ERR_ARG before any device call: everything l2hmc_small_hmc_run refuses, NULL temps, group < 2 or
 * > 64, B not a multiple of group, swap_every < 1, swap_phase outside [0, swap_every), first_parity not 0 or 1,
 * draw0 + 2 n_steps + rounds beyond 2^64 - 1. */
int l2hmc_small_hmc_run_exchange(const l2hmc_small_plan* plan, const float* x_in, float* x_next, int64_t B,
                                 uint64_t seed, uint64_t draw0, int32_t n_steps,
                                 const float* temps, int64_t step_stride, int64_t chain_stride, const float* eps_chain,
                                 int32_t group, int32_t swap_every, int32_t swap_phase, int32_t first_parity,
                                 int32_t* replica, float* px, float* samples,
                                 float* swap_p, uint8_t* swapped, int32_t* replica_hist, l2hmc_stream_t stream);

/* l2hmc_small_run_tempered with replica exchange between the columns of a temperature ladder INSIDE the launch: its
 * contract (an L2HMC plan, the four streams of a step, px, samples, x_next that may alias x_in, temps with its strides,
 * the form the batch size selects, no workspace, graph capture, the same bits on every run, B == 0 a no-op) with these
 * differences.
 * After step s of the launch one round of l2hmc_small_replica_swap (group, the rule and the arithmetic above) runs iff
 * (swap_phase + s + 1) % swap_every == 0, on the state the step left and at the temperatures the step ran with
 * (temps[s * step_stride + c * chain_stride]); the j-th round of the launch has parity (first_parity + j) % 2.
 * Streams are taken in the order of the loop a caller would write: a step takes four (direction bits, forward momenta,
 * backward momenta, Metropolis-Hastings uniforms), a round the next one -- a round without a pair takes its stream as
 * well, so the accounting does not depend on the group size.  The launch consumes streams
 * draw0 .. draw0 + 4 n_steps + rounds - 1, rounds = (swap_phase + n_steps) / swap_every.
 * samples[s] and px[s] are step s's own outputs, taken BEFORE its round; the round shows in the next step's input and
 * in x_next.  replica [B] (int32 labels, or NULL) is read on entry and written on exit.  swap_p, swapped and
 * replica_hist (the labels after each round) are [rounds][B]; each may be NULL.
 * ONE launch (profile class 7, none of class 8) of the run kernel's exchange instances.  The kernel gives a chain eight
 * lanes (four of the matrix instructions times two directions) and a wave eight chains; here a wave holds
 * (8 / group) * group chains, whole groups, so a round is a handful of cross-lane reads between two steps: for group
 * 2, 4, 8 the placement of l2hmc_small_run_tempered, for 3, 5, 6, 7 some of a wave's eight places stay idle and the
 * launch has more waves.  The FORM is still the one l2hmc_small_run_tempered takes for the same plan and B, so the call
 * is bit for bit the loop l2hmc_small_run_tempered (up to the next round), l2hmc_small_replica_swap: both rounds call
 * one device function on the fp32 state the run would store and reload.
 * Refused with L2HMC_ERR_ARG before any device call: everything l2hmc_small_run_tempered refuses, NULL temps, group < 2
 * or > 8 (larger groups would cross waves: they stay with the round between launches), B not a multiple of group,
 * swap_every < 1, swap_phase outside [0, swap_every), first_parity not 0 or 1, draw0 + 4 n_steps + rounds beyond
 * 2^64 - 1. */
int l2hmc_small_run_exchange(const l2hmc_small_plan* plan, const float* x_in, float* x_next, int64_t B,
                             uint64_t seed, uint64_t draw0, int32_t n_steps,
                             const float* temps, int64_t step_stride, int64_t chain_stride,
                             int32_t group, int32_t swap_every, int32_t swap_phase, int32_t first_parity,
                             int32_t* replica, float* px, float* samples,
                             float* swap_p, uint8_t* swapped, int32_t* replica_hist, l2hmc_stream_t stream);

/* One training evaluation on the toy targets (mog_model.py:324-363): `rows` = 2B stacked chains (B started at
 * x, B at z ~ N(0,1); sampler.py:28-55 picks a direction per chain, passed in `dir`), each integrated in its
 * direction; per chain v = |x0 - x_N|^2 * p + 1e-4, term = scale / v - v / scale, loss = inv_count * sum of all
 * 2B terms (inv_count = 1/B).  ONE launch runs forward, loss and the whole reverse pass on-chip.
 * Outputs: x_out, v_out [rows][x_dim] proposals; p_accept, terms [rows]; grads (device, overwritten):
 * [xnet gradient | vnet gradient | d loss / d eps], each network in the flat order
 * [w1_t | wt | b1 | wh_t | bh | whd_t | bhd | coeff_s | coeff_q] of struct l2hmc_dense_net
 * (d loss / d alpha = eps * d loss / d eps, utils/dynamics.py:51-60). */
size_t l2hmc_small_train_ws_bytes(const l2hmc_small_plan* plan, int64_t rows);
int l2hmc_small_train_step(const l2hmc_small_plan* plan, const float* x0, const float* v0, const int32_t* dir,
                           int64_t rows, float scale, float inv_count, float* x_out, float* v_out,
                           float* p_accept, float* terms, float* grads, void* ws, size_t ws_bytes,
                           l2hmc_stream_t stream);
/* l2hmc_small_train_step on a LADDER of temperatures: row r runs at temps[(r % chains) * chain_stride], temps a DEVICE
 * array (the convention of l2hmc_gauge_train_forward_ladder).  With the stacked batch [x | z] of rows = 2 * chains,
 * chain i of x and chain i of z share temps[i]; chain_stride 0 = one value for every row, read from the device.
 * plan->target.temperature is IGNORED.  Everything else -- outputs, the layout and the fixed summation order of grads,
 * the launch geometry, the workspace (l2hmc_small_train_ws_bytes(plan, rows), unchanged) -- is l2hmc_small_train_step's:
 * a row has the bits of that entry at its temperature, and equal temperatures give its gradient buffer bit for bit.
 * Refused with L2HMC_ERR_ARG before any launch: everything l2hmc_small_train_step refuses, NULL temps, chains <= 0,
 * rows that are no whole number of chains, a chain_stride that is negative (or anything but 0 or 1).  The VALUES of
 * temps are on the device and are not checked here (DynamicsTrainer checks them: finite and > 0 in float32). */
int l2hmc_small_train_step_tempered(const l2hmc_small_plan* plan, const float* temps, int64_t chain_stride,
                                    int64_t chains, const float* x0, const float* v0, const int32_t* dir,
                                    int64_t rows, float scale, float inv_count, float* x_out, float* v_out,
                                    float* p_accept, float* terms, float* grads, void* ws, size_t ws_bytes,
                                    l2hmc_stream_t stream);
/* Vector-Jacobian product of l2hmc_small_trajectory for ANY cotangents: what a caller's autograd needs to
 * differentiate a loss of its own through Dynamics.forward / .backward / propose.  Per row r (direction dir[r],
 * NULL = all forward) the forward from (x0, v0) is recomputed on-chip, then the reverse pass of
 * l2hmc_small_train_step runs, seeded with the cotangents g_x, g_v [rows][x_dim] of (x_N, v_N) and g_logdet, g_p
 * [rows] of (sumlogdet, p_accept); each may be NULL (= 0).  With p = min(1, exp(D)), D = H0 - H1 + sumlogdet
 * (NaN D: p = 0), dD = g_p p where p < 1 and 0 otherwise; dD reaches x_N and v_N through -H1, sumlogdet, and the
 * start state through +H0 (dx0 += dD grad E(x0) with the tempered energy, dv0 += dD v0).
 * Outputs: grads (device, overwritten) = [xnet | vnet | d/d eps] in the layout and the fixed summation order of
 * l2hmc_small_train_step (d/d alpha = eps d/d eps); dx0, dv0 [rows][x_dim] the gradients with respect to each row's
 * own start state; x_out, v_out, sumlogdet, p_accept the recomputed forward.  Each of dx0, dv0, x_out, v_out,
 * sumlogdet, p_accept may be NULL (not written).  Same launch geometry as l2hmc_small_train_step, no atomics:
 * reproducible.  Workspace: l2hmc_small_train_ws_bytes(plan, rows). */
int l2hmc_small_vjp(const l2hmc_small_plan* plan, const float* x0, const float* v0, const int32_t* dir,
                    int64_t rows, const float* g_x, const float* g_v, const float* g_logdet, const float* g_p,
                    float* dx0, float* dv0, float* grads, float* x_out, float* v_out, float* sumlogdet,
                    float* p_accept, void* ws, size_t ws_bytes, l2hmc_stream_t stream);
/* l2hmc_small_vjp on a LADDER of temperatures (the reverse of l2hmc_small_trajectory_tempered): row r at
 * temps[(r % chains) * chain_stride], temps a DEVICE array, chain_stride 1 or 0; plan->target.temperature is IGNORED.
 * The direct term dx0 += dD grad E(x0) uses the row's tempered energy.  The VJP instance of the kernel
 * l2hmc_small_train_step_tempered runs: same launch geometry, no atomics, the workspace of
 * l2hmc_small_train_ws_bytes(plan, rows); dx0, dv0 and the recomputed forward of a row have the bits of l2hmc_small_vjp
 * at its temperature, and equal temperatures give its grads buffer bit for bit.  rows == 0 is a no-op after the checks.
 * Refused with L2HMC_ERR_ARG before any launch: NULL temps, a chain_stride other than 0 or 1, chains <= 0,
 * rows % chains != 0, and everything l2hmc_small_vjp refuses.  The VALUES of temps are not checked here. */
int l2hmc_small_vjp_tempered(const l2hmc_small_plan* plan, const float* temps, int64_t chain_stride, int64_t chains,
                             const float* x0, const float* v0, const int32_t* dir, int64_t rows, const float* g_x,
                             const float* g_v, const float* g_logdet, const float* g_p, float* dx0, float* dv0,
                             float* grads, float* x_out, float* v_out, float* sumlogdet, float* p_accept, void* ws,
                             size_t ws_bytes, l2hmc_stream_t stream);

/* Hessian-vector product of the packed target's tempered energy: out[r] = Hess(energy / temperature)(x[r]) . u[r],
 * x, u, out [rows][dim] (the closed form of the second derivative of distributions.py:151-158 / :63-68).  What a
 * reverse pass through VNet([x, grad E(x), t]) needs for the gradient input. */
int l2hmc_mog_energy_hvp(const l2hmc_mog_target* tgt, const float* x, const float* u, int64_t rows, float* out,
                         l2hmc_stream_t stream);

/* out[r] = beta * Hess(S)(x[r]) . u[r] for the 2-D U(1) action S of l2hmc_u1_action_force (whose `force` is
 * beta * dS/dx): the force's stencil with sin(P) replaced by cos(P) * P[u].  x, u, out [rows][2*T*X].  What a reverse
 * pass through VNet([x, force(x), t]) needs for the force input, at any T x X.  One wave per row, the chain and the
 * per-plaquette cos(P) * P[u] staged in LDS (20 bytes per site): a lattice whose row does not fit one workgroup's
 * LDS (more than 8192 sites) is refused.  rows = 0 is a no-op; out must not alias x or u. */
int l2hmc_u1_force_hvp(const float* x, const float* u, int64_t rows, int32_t T, int32_t X, float beta, float* out,
                       l2hmc_stream_t stream);

/* ------------------------------------------------------------------------
 * Training of the layer-by-layer generic Dynamics (any x_dim, num_nodes, energy; mog_model.py:324-363 through
 * utils/dynamics.py:120-225): the building blocks of a taped reverse pass, orchestrated by
 * l2hmc_amd/layered_train.py.  Every entry takes ANY positive D, H, Ka, Kb (bounds-checked loads where widths are
 * not multiples of 32 or rows are not 16-byte aligned); rows = 0 is a no-op.
 * ------------------------------------------------------------------------ */
/* l2hmc_stq_dense with the post-relu activations h1, h2 [rows][H] written to caller buffers instead of the
 * workspace: same kernels, so S, T, Q are bit-identical to l2hmc_stq_dense. */
int l2hmc_stq_dense_taped(const l2hmc_dense_net* net, const float* a, const float* b, const float* bmask,
                          float t_cos, float t_sin, int64_t rows, float* S, float* T, float* Q, float* h1, float* h2,
                          l2hmc_stream_t stream);

/* Vector-Jacobian products of l2hmc_lf_update_v / l2hmc_lf_update_x (utils/dynamics.py:123-223, both directions).
 * dv_out / dx_out [rows][D]: cotangent of the output state; dlogdet [rows]: cotangent of the per-row log-det (may be
 * NULL = 0).  Outputs (overwritten): the cotangents of the input state (dv / dx), of the gradient input (dgrad, v
 * update) or of v (dv, x update: the part through this update only), of S, T, Q [rows][D], and deps [rows], each
 * row's partial d/d eps.  Outputs must not alias inputs. */
int l2hmc_lf_update_v_vjp(const float* v, const float* grad, const float* S, const float* T, const float* Q,
                          float eps, int32_t dir, int64_t rows, int32_t D, const float* dv_out, const float* dlogdet,
                          float* dv, float* dgrad, float* dS, float* dT, float* dQ, float* deps,
                          l2hmc_stream_t stream);
int l2hmc_lf_update_x_vjp(const float* x, const float* v, const float* keep, const float* S, const float* T,
                          const float* Q, float eps, int32_t dir, int64_t rows, int32_t D, const float* dx_out,
                          const float* dlogdet, float* dx, float* dv, float* dS, float* dT, float* dQ, float* deps,
                          l2hmc_stream_t stream);

/* The same for l2hmc_lf_update_x_ncp. */
int l2hmc_lf_update_x_ncp_vjp(const float* x, const float* v, const float* keep, const float* S, const float* T,
                              const float* Q, float eps, int32_t dir, int64_t rows, int32_t D, const float* dx_out,
                              const float* dlogdet, float* dx, float* dv, float* dS, float* dT, float* dQ, float* deps,
                              l2hmc_stream_t stream);

/* Backward-data of one network call.  Input: the call's S, Q, the cotangents dS, dT, dQ [rows][D] and its taped
 * h1, h2 [rows][H].  Outputs: dpre [rows][3D] the head pre-activation cotangents (tanh' and exp(coeff) applied),
 * dsq [rows][2D] = [dS * S | dQ * Q] (the per-row coefficient gradients; may be NULL), dz2, dz1 [rows][H] the
 * pre-activation cotangents of the hidden layers (relu-gated), din [rows][Ka+Kb] = [d/da | d/db] of the network
 * inputs.  Workspace (transposed weights): l2hmc_dense_backward_data_ws_bytes(net). */
size_t l2hmc_dense_backward_data_ws_bytes(const l2hmc_dense_net* net);
int l2hmc_dense_backward_data(const l2hmc_dense_net* net, const float* S, const float* Q, const float* dS,
                              const float* dT, const float* dQ, const float* h1, const float* h2, int64_t rows,
                              float* dpre, float* dsq, float* dz2, float* dz1, float* din, void* ws, size_t ws_bytes,
                              l2hmc_stream_t stream);

/* Weight gradients of one network over R taped rows (all its calls stacked along rows): in [R][Ka+Kb] the network
 * inputs [a | b], h1, h2, dz1, dz2 [R][H], dpre [R][3D], dsq [R][2D] as above, tcs [R][2] each row's (cos, sin) time
 * input.  g (overwritten) gets w1_t, wt, b1, wh_t, bh, whd_t, bhd, coeff_s, coeff_q in the layout of struct
 * l2hmc_dense_net.  Split-k products and column sums, every reduction in a fixed order (no float atomics): two calls
 * give the same bits.  Workspace: l2hmc_dense_weight_grads_ws_bytes(net, R). */
size_t l2hmc_dense_weight_grads_ws_bytes(const l2hmc_dense_net* net, int64_t R);
int l2hmc_dense_weight_grads(const l2hmc_dense_net* net, int64_t R, const float* in, const float* h1,
                             const float* h2, const float* dz1, const float* dz2, const float* dpre, const float* dsq,
                             const float* tcs, const l2hmc_dense_grads* g, void* ws, size_t ws_bytes,
                             l2hmc_stream_t stream);

/* ------------------------------------------------------------------------
 * Counter-based RNG (Philox4x32-10) standing in for tf.random_normal /
 * tf.random_uniform (gauge_dynamics.py:223,246,269).  Same (seed, offset, n)
 * => same stream on any launch geometry.
 * ------------------------------------------------------------------------ */
int l2hmc_fill_normal(float* out, int64_t n, uint64_t seed, uint64_t offset, l2hmc_stream_t stream);
int l2hmc_fill_uniform(float* out, int64_t n, uint64_t seed, uint64_t offset, l2hmc_stream_t stream);

/* ------------------------------------------------------------------------
 * Measurement aid (no reference counterpart): time every launch of one kernel
 * class with HIP events recorded on the launch stream.  begin() arms it (0
 * disarms), end() synchronises the recorded events and returns the summed
 * kernel time and launch count.  One process-wide recorder (mutex-protected; launches of concurrent threads are
 * recorded one after the other); not for use while capturing a graph.
 *   1 = first dense layer   2 = hidden dense layer   3 = heads (+update)
 *   4 = u1_action_force     5 = fused whole-trajectory kernel
 *   6 = ConvNet3D front-end 7 = toy-target trajectory kernel (l2hmc_small_*)
 *   8 = replica-exchange round on its own (l2hmc_gauge_replica_swap, l2hmc_small_replica_swap; the rounds inside
 *       l2hmc_small_hmc_run_exchange and l2hmc_small_run_exchange are part of their class-7 launch, those inside
 *       l2hmc_gauge_hmc_run_exchange of its class-5 launch)
 * ------------------------------------------------------------------------ */
int l2hmc_profile_begin(int32_t kernel_class);
int l2hmc_profile_end(double* total_ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* L2HMC_HIP_H */
