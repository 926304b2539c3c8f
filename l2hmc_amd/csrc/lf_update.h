// The arithmetic of one leapfrog sub-update, per element, and of its reverse: the ONE copy every kernel calls
// (gauge_dynamics.py:486-590, utils/dynamics.py:120-225).  With h = eps / 2:
//   momentum  s = +-h S,    kick  = h (e^{eps Q} g - T),      v' = v e^s - kick  (dir 0),  e^s (v + kick)   (dir 1)
//   position  s = +-eps S,  drift = eps (e^{eps Q} v + T),    y  = x e^s + drift (dir 0),  e^s (x - drift)  (dir 1)
//             x' = keep x + (1 - keep) y,   log-det term (1 - keep) s
// Loads, stores, vectorisation, staging for the next call, tapes and cross-lane sums stay at the call sites.
//
// The build contracts a multiply into an add WITHIN a statement only (-ffp-contract=on), so statement boundaries
// decide the bits.  The helpers therefore return the FACTORS of every product a site adds into an accumulator of its
// own (s and 1 - keep; dT and e^{eps Q}): `ld += omk * s` at the site stays one fused multiply-add, where a helper that
// returned the rounded product would not.  Sums that are the helper's own (deps) take the accumulator by reference.
//
// Hand copies that remain, because their statements differ from these: the reverse inside gauge_train_bwd_fused_kernel
// (fused_train.hip: fast_exp, and the backward kick folded into vp's statement) and small_train.hip's momentum reverse
// (the same folded statement).  fused_traj32.hip spells keep_of's expression out at its position update (there the
// call costs the 256-VGPR kernel one more spilled register).
#pragma once
#include "common.h"

namespace l2hmc {

// which exponential a site uses: libm's (standalone operators, training forward passes) or the hardware exp2 form
struct ExpLibm { static __device__ __forceinline__ float f(float x) { return expf(x); } };
struct ExpFast { static __device__ __forceinline__ float f(float x) { return fast_exp(x); } };

// (S, T, Q) from the three head products of one column (generic_net.py:139-144); e_s = e^{coeff_s}, e_q = e^{coeff_q}
__device__ __forceinline__ void heads_stq(float aS, float aT, float aQ, float b_s, float b_t, float b_q, float e_s,
                                          float e_q, int q_tanh, float& S, float& T, float& Q) {
  S = fast_tanh(aS + b_s) * e_s;
  T = aT + b_t;
  const float qq = aQ + b_q;
  Q = (q_tanh ? fast_tanh(qq) : qq) * e_q;
}

// keep mask of position sub-update `sub` (0, 1) in direction d from the forward step's mask value mf and the backward
// step's mb: forward (m, 1 - m), backward (1 - m, m)   (gauge_dynamics.py:428-438, :466-476)
__device__ __forceinline__ float keep_of(float mf, float mb, int d, int sub) {
  return sub == 0 ? (d ? 1.f - mb : mf) : (d ? mb : 1.f - mf);
}

// momentum sub-update: returns v'; s is the element's log-det term
template <class Exp>
__device__ __forceinline__ float lf_kick(float v, float g, float S, float T, float Q, float eps, int d, float& s) {
  s = (d ? -0.5f : 0.5f) * eps * S;
  const float kick = 0.5f * eps * (Exp::f(eps * Q) * g - T);
  const float es = Exp::f(s);
  return d ? es * (v + kick) : v * es - kick;
}

// position sub-update: returns x'; the element's log-det term is omk * s with omk = 1 - keep
template <class Exp>
__device__ __forceinline__ float lf_drift(float x, float v, float keep, float S, float T, float Q, float eps, int d,
                                          float& s, float& omk) {
  s = (d ? -eps : eps) * S;
  const float drift = eps * (Exp::f(eps * Q) * v + T);
  const float es = Exp::f(s);
  const float upd = d ? es * (x - drift) : x * es + drift;
  omk = 1.f - keep;
  return keep * x + omk * upd;
}

// position sub-update of the torus-exact mode (L2HMC_PLAN_PERIODIC): the scaling x e^s of lf_drift becomes the map of
// the circle onto itself  x -> 2 atan2(e^s sin(x / 2), cos(x / 2)),  whose derivative is e^s / r2 with
// r2 = cos^2(x / 2) + e^{2s} sin^2(x / 2).  With w = x (dir 0) or x - drift (dir 1):
//   y = 2 atan2(e^s sin(w / 2), cos(w / 2)) [+ drift, dir 0],   x' = keep x + (1 - keep) y   (principal value of atan2)
// Returns x'; the element's log-det term is omk * s, where s here is +-eps S - log r2 (the same site statement as
// lf_drift's).  sin, cos, atan2 and log are libm's in every site: only the exponentials follow Exp.
template <class Exp>
__device__ __forceinline__ float lf_drift_ncp(float x, float v, float keep, float S, float T, float Q, float eps, int d,
                                              float& s, float& omk) {
  const float se = (d ? -eps : eps) * S;
  const float drift = eps * (Exp::f(eps * Q) * v + T);
  const float es = Exp::f(se);
  const float w = d ? x - drift : x;
  float sh, ch;
  sincosf(0.5f * w, &sh, &ch);
  const float a = es * sh;
  const float y = 2.f * atan2f(a, ch);
  const float upd = d ? y : y + drift;
  s = se - logf(ch * ch + a * a);
  omk = 1.f - keep;
  return keep * x + omk * upd;
}

// reverse of lf_kick<ExpLibm>: u = d/dv', dl = d/dlogdet -> cotangents of v, g, S, T, Q; deps += d/deps
__device__ __forceinline__ void lf_kick_vjp(float v, float g, float S, float T, float Q, float eps, int d, float u,
                                            float dl, float& dv, float& dg, float& dS, float& dT, float& dQ,
                                            float& deps) {
  const float he = 0.5f * eps;
  const float eq = expf(eps * Q);
  if (!d) {
    const float es = expf(he * S);
    const float ds = u * v * es + dl;
    dv = u * es;
    dS = ds * he; dT = u * he; dQ = -u * he * eq * g * eps;
    dg = -u * he * eq;
    deps += ds * 0.5f * S - u * 0.5f * (eq * g - T) - u * he * g * eq * Q;
  } else {
    const float es = expf(-he * S);
    const float kick = he * (eq * g - T);
    const float vp = es * (v + kick);
    const float dw = u * es;
    const float ds = u * vp + dl;
    dv = dw;
    dS = -he * ds; dT = -dw * he; dQ = dw * he * eq * g * eps;
    dg = dw * he * eq;
    deps += -0.5f * S * ds + dw * 0.5f * (eq * g - T) + dw * he * g * eq * Q;
  }
}

// reverse of lf_drift<ExpLibm>: u = d/dx', dl = d/dlogdet -> cotangents of x, S, T, Q; deps += d/deps.  The cotangent
// of v through this update is dT * eq (eq = e^{eps Q}): the site stores it or adds it into its own dv in one statement
__device__ __forceinline__ void lf_drift_vjp(float x, float v, float keep, float S, float T, float Q, float eps, int d,
                                             float u, float dl, float& dx, float& dS, float& dT, float& dQ, float& eq,
                                             float& deps) {
  const float mi = 1.f - keep;
  eq = expf(eps * Q);
  const float dy = mi * u;
  if (!d) {
    const float es = expf(eps * S);
    const float ds = dy * x * es + dl * mi;
    dx = keep * u + dy * es;
    dS = eps * ds; dT = dy * eps; dQ = dy * eps * eq * v * eps;
    deps += ds * S + dy * (eq * v + T) + dy * eps * v * eq * Q;
  } else {
    const float es = expf(-eps * S);
    const float w = x - eps * (eq * v + T);
    const float dw = dy * es;
    const float ds = dy * (es * w) + dl * mi;
    dx = keep * u + dw;
    dS = -eps * ds; dT = -dw * eps; dQ = -dw * eps * eq * v * eps;
    deps += -S * ds - dw * (eq * v + T) - dw * eps * v * eq * Q;
  }
}

// reverse of lf_drift_ncp<ExpLibm>, with lf_drift_vjp's conventions (the cotangent of v is dT * eq).  With h = w / 2,
// a = e^s sin h, c = cos h, r2 = c^2 + a^2:  dy/dw = e^s / r2,  dy/ds = 2 a c / r2,  and for the log-det term
// L = s - log r2:  dL/dw = -sin h cos h (e^{2s} - 1) / r2,  dL/ds = 1 - 2 a^2 / r2
__device__ __forceinline__ void lf_drift_ncp_vjp(float x, float v, float keep, float S, float T, float Q, float eps,
                                                 int d, float u, float dl, float& dx, float& dS, float& dT, float& dQ,
                                                 float& eq, float& deps) {
  const float mi = 1.f - keep;
  eq = expf(eps * Q);
  const float es = expf((d ? -eps : eps) * S);
  const float w = d ? x - eps * (eq * v + T) : x;
  float sh, ch;
  sincosf(0.5f * w, &sh, &ch);
  const float a = es * sh;
  const float ir = 1.f / (ch * ch + a * a);
  const float dy = mi * u, dL = dl * mi;
  const float dw = dy * es * ir - dL * sh * ch * (es * es - 1.f) * ir;
  const float ds = dy * 2.f * a * ch * ir + dL * (1.f - 2.f * a * a * ir);
  dx = keep * u + dw;
  if (!d) {
    dS = eps * ds; dT = dy * eps; dQ = dy * eps * eq * v * eps;
    deps += ds * S + dy * (eq * v + T) + dy * eps * v * eq * Q;
  } else {
    dS = -eps * ds; dT = -dw * eps; dQ = -dw * eps * eq * v * eps;
    deps += -S * ds - dw * (eq * v + T) - dw * eps * v * eq * Q;
  }
}

}  // namespace l2hmc
