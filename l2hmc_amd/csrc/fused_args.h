// Launch descriptor of the whole-trajectory kernels (fused_traj.hip: 16 rows per workgroup; fused_traj4.hip: the
// sub-tile form for batches that cannot fill 16-row tiles on every CU).
#pragma once
#include "stq_dense.h"

namespace l2hmc {

struct FusedArgs {
  int T, X, num_steps, step_begin, step_end;
  float eps, beta;
  const float* masks;                    // [num_steps][D]
  l2hmc_dense_net xnet, vnet;            // .packed must be set
  l2hmc_conv3d_front xfront, vfront;     // ConvNet3D only
  const float* x0; const float* v0;      // [rows][D]
  const int* dir;                        // [rows] or NULL
  int64_t x_mod;                         // > 0: row r starts from x0[r % x_mod] (both directions of one batch)
  int64_t dir_split;                     // dir == NULL and > 0: rows >= dir_split integrate backward
  int64_t rows;
  float* x_out; float* v_out;            // [rows][D]
  float* logdet;                         // [rows] or NULL; written (=) or accumulated (+=)
  int logdet_accumulate;
  float* p_accept;                       // [rows] or NULL
  unsigned long long* stamps;            // diagnostic builds only
  int stagger;                           // cycles of start delay per in-XCD workgroup index (0 = none)
  FusedTape tx, tv;                      // training tape per network (all-NULL = sampling)
  // Whole-MCMC-step mode (l2hmc_gauge_mcmc_step, l2hmc_gauge_transition_draw; step_B > 0): the kernel draws its own momenta / coin /
  // MH uniform (Philox streams (seed, 2 draw) and (seed, 2 draw + 1), bit-identical to l2hmc_fill_*), integrates,
  // mixes, accepts, measures and wraps -- ONE launch per MCMC step.  A workgroup then owns 8 chains x both
  // directions (rows 0-7 forward, 8-15 backward of the same chains) or, with step_both = 0, 16 chains in the
  // direction their coin selects; x0 = the step's input samples [B][D], v0 / dir / x_out / v_out are unused.
  float* step_x_next;                    // [B][D] wrapped output samples (may alias x0), or NULL
  float* step_xprop; float* step_vprop; float* step_xout;   // [B][D] apply_transition's outputs (unwrapped), or NULL
  int64_t step_B;                        // > 0 switches the mode on: chains of the WHOLE batch (Philox stream offsets, count)
  int64_t step_Bl, step_chain0;          // chains of THIS launch and the first one's index in the batch; the per-chain
                                         // pointers (x0, step_x_next, step_px, ...) are already moved to that chain
  int step_sums_acc;                     // 1: add this launch's sums to step_sums (second launch of a batch cut in two)
  unsigned long long step_seed, step_draw;
  int step_both;
  float* step_px; float* step_act; float* step_plq; float* step_chg; float* step_dq;   // [B] each, or NULL
  float* step_sums;                      // [4] = [sum p, sum |dQ|, B, ticket] or NULL; ticket 0 on entry, left 0
  float* step_part;                      // [2 * workgroups] scratch for the fixed-order sums
  // step_both on the 16-row GenericNet form: step_split = 1 gives every workgroup 16 chains of ONE direction --
  // workgroup 2 i integrates chains [16 i, 16 i + 16) forward, workgroup 2 i + 1 the same chains backward -- so that a
  // position sub-update can form its heads on the columns its (uniform) mask moves.  Both leave their rows in
  // step_hand and take the pair's ticket; the one that arrives last mixes, accepts and measures the 16 chains.
  int step_split;
  float* step_hand;                      // [workgroups][2 * 16 * D + 16]: x rows, v rows, accept probabilities
  int* step_ticket;                      // [workgroups / 2], zero on entry (a clear kernel ahead of the launch), left 0
  const int* heads_meta;                 // l2hmc_gauge_pack_heads image (step_split only), or NULL = all columns:
  const float* heads_img;                //   [N][2] eligibility, [N][2][D / 2] columns, [N][D] compact k; [N][2] packed heads sections
  const float* l1_img;                   // its [N][2] kept-column first-layer sections (needs heads_img), or NULL = full K
  int single_kicks;                      // 16-row GenericNet sampling form: every momentum half-kick a network call of its own
                                         // (L2HMC_PLAN_SINGLE_KICKS); 0 = step s's second and step s + 1's first as one pass
  // A ladder of beta in step mode (l2hmc_gauge_mcmc_step_ladder; the LADDER instances of the kernels, launched iff
  // step_betas is set): chain c of the launch runs at step_betas[c * step_beta_stride] -- a DEVICE pointer, moved to
  // the launch's first chain like the other per-chain pointers; element stride 0 or 1.  NULL: `beta` for every chain.
  // (Last in the struct: the uniform instances read what they read before, at the offsets they read it from.)
  const float* step_betas;
  int64_t step_beta_stride;
  // The same two fields in TRAJECTORY mode, for the taped forward of a training step on a ladder
  // (l2hmc_gauge_train_forward_ladder; the TAPE && LADDER instances): row r of the launch runs at
  // step_betas[(r % step_beta_mod) * step_beta_stride] -- RowBeta's rule, so rows i and B + i of the stacked x and z
  // chains share chain i's value.  Read by those instances only.
  int64_t step_beta_mod;
};

// the sub-tile form (fused_traj4.hip): GenericNet 8x8 plans, sampling only
size_t fused4_pack_floats(const l2hmc_dense_net* n);                 // floats of its weight image (appended to the 16-row image)
int launch_fused4_pack(const l2hmc_dense_net* n, float* image4, hipStream_t stream);
int fused4_rows_per_wg(int64_t rows, int cus);                       // 0: use the 16-row form; else 4, 8 or 12 (at most one workgroup per CU)
int launch_fused4(const FusedArgs& a, int rows_per_wg, hipStream_t stream);

// the 32-row form (fused_traj32.hip): same plans, same packed image as the 16-row form; for batches of more than one
// round of 16-row workgroups (each weight fragment then feeds two MFMAs)
int fused32_supported(const l2hmc_dense_net* n);
int launch_fused32(const FusedArgs& a, hipStream_t stream);

// the torus-exact mode's whole-step kernel (fused_traj_ncp.hip): plans with L2HMC_PLAN_PERIODIC and
// L2HMC_PLAN_PERIODIC_STEP on D = 128, one 16-row form for every batch; reads the 4-wave image of l2hmc_dense_pack.
// recompute: form every first-layer product anew (L2HMC_PLAN_RECOMPUTE)
int fused_ncp_net_supported(const l2hmc_dense_net* n);
int fused_ncp_plan(const l2hmc_gauge_plan* p);
// FusedArgs::tx / tv set: its taped instances (trajectory mode, a beta per row with step_beta_mod), the training forward
// of the plans fused_ncp_tape_plan (stq_dense.h) accepts
int launch_fused_ncp(const FusedArgs& a, int recompute, hipStream_t stream);

}  // namespace l2hmc
