// Batched per-group ARIMAX fit, fitted values and forecast for gfx950
// (MI355X).
//
// One statsmodels fit per group becomes a fixed-schedule estimator (see
// forecast/batched.py, the numpy oracle these kernels are tested against):
//   stage 0: w = diff^d(y), centered with its mean wm
//   stage 1: OLS regression on the shared exog design -> per-group beta
//            (precomputed by ops/csrc/mfma_project.hip, or in the kernel)
//   stage 2: Yule-Walker + Levinson-Durbin long-AR -> innovations
//   stage 3: lag-matrix normal equations (<= 8x8), ridge + Cholesky,
//            stationarity shrinkage; one refinement pass (stage 4)
//   stage 5: H-step forecast, integrated to y-units
//
// ONE GROUP PER LANE, 64 groups per wave, one wave per workgroup. Global
// series are TIME-MAJOR [T][G], so every per-timestep access is a fully
// coalesced 64-lane load.
//
// Nothing of length T is stored. Every stage looks back at most 8 lags, so
// each pass re-derives u_t from the y stream (one coalesced load + KX fma)
// and carries 8-deep per-lane REGISTER rings, constant-indexed under full
// unrolls (a runtime-indexed register array goes to scratch). The only
// per-lane memory is the LDS state block of the fit's small matrices and
// vectors (120 floats x 64 lanes = 30 KB), which bounds the fit kernels at
// 5 waves per CU; the forecast kernel holds its coefficients in registers
// and uses no LDS. The y re-reads are cheap: about 4 passes x n x 4 B x G
// per candidate.
//
// Three kernels share the pieces below: groupfit_eval_kernel (every group
// x every candidate order -> validation MSE), groupfit_final_kernel (one
// order per group on the whole series -> fitted values + coefficients)
// and groupfit_forecast_kernel (stored coefficients -> forecast + standard
// errors). The matrix cores only help stage 1; the per-group normal
// equations are at most 8x8 over ~120 steps and latency-bound.

#include <hip/hip_runtime.h>
#include <math.h>

#include "groupfit.h"

#define WAVE 64
#define MAXK 8          // p + q <= 8, KX <= 8
#define MAXM 7          // long-AR order cap
#define RIDGE 1e-6f
#define SHRINK 0.98f

// per-lane LDS state layout (floats), stride WAVE
#define ST_A 0          // 8x8 normal-equation matrix (row-major)
#define ST_C 64         // rhs / solution (8)
#define ST_R 72         // autocovariances (8)
#define ST_AL 80        // long-AR coefs (8)
#define ST_TMP 88       // levinson scratch (8)
#define ST_BETA 96      // exog coefs (8)
#define ST_PHI 104      // AR coefs (4)
#define ST_THETA 108    // MA coefs (4)
#define ST_Z 112        // lag-regressor vector (8)
#define NSTATE 120

#define SIDX(k) ((k) * WAVE + lane)
#define PHI(i) st[SIDX(ST_PHI + (i))]
#define THETA(i) st[SIDX(ST_THETA + (i))]
#define BETA(k) st[SIDX(ST_BETA + (k))]

// Cholesky solve (per-lane LDS): A x = b, A KxK SPD at ST_A, b at ST_C on
// entry, x at ST_C on exit. Runtime K <= 8.
__device__ void chol_solve(float* st, int lane, int K) {
  for (int k = 0; k < K; ++k) {
    float akk = st[SIDX(ST_A + k * 8 + k)];
    for (int j = 0; j < k; ++j) {
      float lkj = st[SIDX(ST_A + k * 8 + j)];
      akk -= lkj * lkj;
    }
    akk = sqrtf(fmaxf(akk, 1e-20f));
    st[SIDX(ST_A + k * 8 + k)] = akk;
    float inv = 1.0f / akk;
    for (int i = k + 1; i < K; ++i) {
      float v = st[SIDX(ST_A + i * 8 + k)];
      for (int j = 0; j < k; ++j)
        v -= st[SIDX(ST_A + i * 8 + j)] * st[SIDX(ST_A + k * 8 + j)];
      st[SIDX(ST_A + i * 8 + k)] = v * inv;
    }
  }
  for (int i = 0; i < K; ++i) {
    float v = st[SIDX(ST_C + i)];
    for (int j = 0; j < i; ++j)
      v -= st[SIDX(ST_A + i * 8 + j)] * st[SIDX(ST_C + j)];
    st[SIDX(ST_C + i)] = v / st[SIDX(ST_A + i * 8 + i)];
  }
  for (int i = K - 1; i >= 0; --i) {
    float v = st[SIDX(ST_C + i)];
    for (int j = i + 1; j < K; ++j)
      v -= st[SIDX(ST_A + j * 8 + i)] * st[SIDX(ST_C + j)];
    st[SIDX(ST_C + i)] = v / st[SIDX(ST_A + i * 8 + i)];
  }
}

// Levinson-Durbin: AR(M) from autocovariances at ST_R -> coefs at ST_AL.
__device__ void levinson(float* st, int lane, int M) {
  for (int i = 0; i < MAXM + 1; ++i) st[SIDX(ST_AL + i)] = 0.0f;
  float e = st[SIDX(ST_R + 0)];
  e = (e > 0.0f) ? e : 1.0f;
  for (int k = 1; k <= M; ++k) {
    float acc = st[SIDX(ST_R + k)];
    for (int j = 0; j < k - 1; ++j)
      acc -= st[SIDX(ST_AL + j)] * st[SIDX(ST_R + (k - 1 - j))];
    float lam = acc / e;
    for (int j = 0; j < k - 1; ++j) st[SIDX(ST_TMP + j)] = st[SIDX(ST_AL + j)];
    for (int j = 0; j < k - 1; ++j)
      st[SIDX(ST_AL + j)] =
          st[SIDX(ST_TMP + j)] - lam * st[SIDX(ST_TMP + (k - 2 - j))];
    st[SIDX(ST_AL + (k - 1))] = lam;
    e *= (1.0f - lam * lam);
    if (e <= 0.0f) e = 1e-12f;
  }
}

// ---------------------------------------------------------------------
// The pieces of the recursion, each written once. With td = t - d:
//   w_t  = diff^d(y)_t                      (diff_step, groupfit.h)
//   u_td = (w_t - wm) - x_td . beta
// and ur[j] = u_{td-1-j}, er[j] = e_{td-1-j} are the register rings
// (zero-filled: pre-sample lags are zero, matching the oracle).
// ---------------------------------------------------------------------

#define RING_SHIFT(r, v)                        \
  _Pragma("unroll") for (int _j = 7; _j > 0; --_j) r[_j] = r[_j - 1]; \
  r[0] = (v)

__device__ __forceinline__ void rings_clear(float* ur, float* er) {
#pragma unroll
  for (int j = 0; j < 8; ++j) { ur[j] = 0.0f; er[j] = 0.0f; }
}

// A lane's order, clamped to what the state block and the rings hold
// (p, q <= 4, d <= 2). The host rejects anything else; for an order that
// reaches a kernel through a device tensor the clamp turns an
// out-of-bounds write into a well-defined wrong answer.
struct Order { int p, d, q; };
__device__ __forceinline__ Order load_order(const int* __restrict__ o) {
  return {min(max(o[0], 0), 4), min(max(o[1], 0), 2), min(max(o[2], 0), 4)};
}

// The operand a{d} of differencing order d. A select, not an array: a
// runtime-indexed array of pointers would go to scratch. A macro, not a
// function: selected inside an inlined helper, the forecast kernel
// allocates 66 VGPRs instead of 64 and loses a wave per SIMD.
#define PICK_D(d, a) (((d) == 0) ? a##0 : ((d) == 1) ? a##1 : a##2)

// The lane's beta in the LDS state block.
struct LdsBeta {
  const float* st;
  int lane;
};

// Regression term x_row . beta of design row `row`, summed from 0 for
// k = 0..KX-1. Two loop shapes for the two homes of beta: a runtime trip
// count over LDS, and a full unroll with a predicate over registers, which
// keeps the register array constant-indexed.
__device__ __forceinline__ float reg_term(const float* __restrict__ xc,
                                          long long row, const LdsBeta& b,
                                          int KX) {
  const float* st = b.st;
  const int lane = b.lane;
  float reg = 0.0f;
  for (int k = 0; k < KX; ++k) reg += xc[row * KX + k] * BETA(k);
  return reg;
}
__device__ __forceinline__ float reg_term(const float* __restrict__ xc,
                                          long long row,
                                          const float (&beta)[MAXK],
                                          int KX) {
  float reg = 0.0f;
#pragma unroll
  for (int k = 0; k < MAXK; ++k)
    if (k < KX) reg += xc[row * KX + k] * beta[k];
  return reg;
}

__device__ __forceinline__ void load_arma(const float* st, int lane,
                                          float* ph, float* th) {
#pragma unroll
  for (int i = 0; i < 4; ++i) { ph[i] = PHI(i); th[i] = THETA(i); }
}

// ARMA part of the prediction from the lag rings (coefs past p, q are 0).
__device__ __forceinline__ float arma_dot(const float* ph, const float* th,
                                          const float* ur, const float* er) {
  return ph[0] * ur[0] + ph[1] * ur[1] + ph[2] * ur[2] + ph[3] * ur[3] +
         th[0] * er[0] + th[1] * er[1] + th[2] * er[2] + th[3] * er[3];
}

// The innovation exists in two roundings, and each kernel keeps its own.
// The fit (NE pass 1 and the final innovation pass of fit_lane) subtracts
// term by term, as the oracle's _fit_arma_one does:
__device__ __forceinline__ float innovation(float u, const float* ph,
                                            const float* th,
                                            const float* ur,
                                            const float* er) {
  float e = u;
#pragma unroll
  for (int i = 0; i < 4; ++i) e -= ph[i] * ur[i] + th[i] * er[i];
  return e;
}
// The fitted-value pass and the forecast's streaming pass need the
// prediction acc itself and take e = u - acc from it. One in-sample step:
// predicts from the lags, THEN pushes the current u and e. Returns e.
__device__ __forceinline__ float insample_step(float w, float wm, float regx,
                                               const float* ph,
                                               const float* th, float* ur,
                                               float* er, float& acc) {
  acc = arma_dot(ph, th, ur, er);
  const float u = (w - wm) - regx;
  const float e = u - acc;
  RING_SHIFT(ur, u);
  RING_SHIFT(er, e);
  return e;
}

// One out-of-sample step in w-space at design row `row`: the future u is
// the ARMA part, the future e is 0. Returns w_pred.
template <class Beta>
__device__ __forceinline__ float forecast_step(const float* __restrict__ xc,
                                               long long row,
                                               const Beta& beta, int KX,
                                               float wm, const float* ph,
                                               const float* th, float* ur,
                                               float* er) {
  const float regx = reg_term(xc, row, beta, KX);
  const float acc = arma_dot(ph, th, ur, er);
  RING_SHIFT(ur, acc);
  RING_SHIFT(er, 0.0f);
  return wm + regx + acc;
}

// Streaming-pass skeleton: walks t = 0..S-1 of one lane's series from a
// zeroed y ring, skips the d warm-up steps and calls body(td, w_td).
template <class Body>
__device__ __forceinline__ void stream_w(const float* __restrict__ yT,
                                         long long g, long long G, int S,
                                         int d, Body body) {
  float y0 = 0.0f, y1 = 0.0f;
  for (int t = 0; t < S; ++t) {
    const float w = diff_step(d, yT[(long long)t * G + g], y0, y1);
    if (t >= d) body(t - d, w);
  }
}

// Core fit for one (group-lane, order): leaves ST_BETA/ST_PHI/ST_THETA
// state and the end-of-series rings ur/er (u_{n-1-j}, e_{n-1-j}).
// *ok_out false on non-finite state.
__device__ float fit_lane(
    const float* __restrict__ yT, const float* __restrict__ xc,
    const float* __restrict__ PJ, float* st,
    int lane, long long g, long long G, int S, int KX, int p, int d, int q,
    bool* ok_out, float* ur, float* er,
    const float* __restrict__ beta_pre,  // [KX][G] from the MFMA
    const float* __restrict__ wm_pre) {  // [G]     projection, or null
  const int n = S - d;

  // ---- stage 0: mean of the differenced series (pass only if needed)
  float wm;
  if (wm_pre) {
    wm = wm_pre[g];
  } else {
    float wsum = 0.0f;
    stream_w(yT, g, G, S, d, [&](int, float w) { wsum += w; });
    wm = wsum / (float)n;
  }

  // ---- stage 1: beta = P @ (w - wm) (pass only if not precomputed)
#pragma unroll
  for (int k = 0; k < MAXK; ++k) BETA(k) = 0.0f;
  if (beta_pre) {
    for (int k = 0; k < KX; ++k) BETA(k) = beta_pre[(long long)k * G + g];
  } else {
    float bacc[MAXK];
#pragma unroll
    for (int k = 0; k < MAXK; ++k) bacc[k] = 0.0f;
    stream_w(yT, g, G, S, d, [&](int td, float w) {
      const float wcv = w - wm;
#pragma unroll
      for (int k = 0; k < MAXK; ++k)
        if (k < KX) bacc[k] += PJ[(long long)k * n + td] * wcv;
    });
#pragma unroll
    for (int k = 0; k < MAXK; ++k)
      if (k < KX) BETA(k) = bacc[k];
  }

  // every later pass streams u_td under the beta just stored
  const LdsBeta beta{st, lane};
  auto stream_u = [&](auto body) {
    stream_w(yT, g, G, S, d, [&](int td, float w) {
      body(td, (w - wm) - reg_term(xc, td, beta, KX));
    });
  };

#pragma unroll
  for (int i = 0; i < 4; ++i) { PHI(i) = 0.0f; THETA(i) = 0.0f; }
  rings_clear(ur, er);

  const int K = p + q;
  const bool lane_q = q > 0;
  const bool lane_K = K > 0;
  int M = 0;

  // ---- stage 2: autocovariance pass + Levinson (q > 0 lanes)
  if (__any(lane_q)) {
    M = max(p, q) + 3;
    if (M > MAXM) M = MAXM;
    if (M > n / 4) M = max(1, n / 4);
    float r[MAXM + 1];
#pragma unroll
    for (int k = 0; k <= MAXM; ++k) r[k] = 0.0f;
    stream_u([&](int, float u) {
      r[0] += u * u;
#pragma unroll
      for (int k = 1; k <= MAXM; ++k)
        if (k <= M) r[k] += u * ur[k - 1];
      RING_SHIFT(ur, u);
    });
    if (lane_q) {
#pragma unroll
      for (int k = 0; k <= MAXM; ++k)
        if (k <= M) st[SIDX(ST_R + k)] = r[k] / (float)n;
      levinson(st, lane, M);
    }
  }

  // ---- stages 3+4: two normal-equation passes + final innovation pass.
  //   NE pass 0: e = long-AR innovations (q>0) / e = u (q==0)
  //   NE pass 1: e = recursive innovations under pass-0 coefs (q>0 only)
  //   final pass: e under final coefs -> end-of-series rings (q>0 only;
  //               q==0 lanes' rings are complete after NE pass 0 and the
  //               theta terms they feed are zero)
  const bool any_q = __any(lane_q);
  if (__any(lane_K)) {
    const int m = max(max(p, q), 1);
    // q==0 lanes solve only in pass 0, and a pure-AR wave needs neither
    // the refinement pass nor the final innovation pass (its theta
    // terms are zero, so the e-ring is never consumed)
    const int npass = any_q ? 2 : 1;
    float phr[4], thr[4];
    for (int pass = 0; pass < npass; ++pass) {
      const bool solve_here = lane_K && (pass == 0 || lane_q);
      // coefs for this pass's innovation recursion
      float alr[MAXM];
#pragma unroll
      for (int i = 0; i < MAXM; ++i)
        alr[i] = (lane_q && pass == 0 && i < M) ? st[SIDX(ST_AL + i)] : 0.0f;
      load_arma(st, lane, phr, thr);
      if (solve_here) {
        for (int i = 0; i < 64; ++i) st[SIDX(ST_A + i)] = 0.0f;
        for (int i = 0; i < 8; ++i) st[SIDX(ST_C + i)] = 0.0f;
      }
      rings_clear(ur, er);
      stream_u([&](int td, float u) {
        // innovation under this pass's recursion
        float e;
        if (pass == 0) {
          e = u;
#pragma unroll
          for (int i = 0; i < MAXM; ++i) e -= alr[i] * ur[i];
        } else {
          e = innovation(u, phr, thr, ur, er);
        }
        if (solve_here && td >= m) {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (i < p) st[SIDX(ST_Z + i)] = ur[i];
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (j < q) st[SIDX(ST_Z + p + j)] = er[j];
          for (int i = 0; i < K; ++i) {
            const float zi = st[SIDX(ST_Z + i)];
            for (int j = i; j < K; ++j)
              st[SIDX(ST_A + i * 8 + j)] += zi * st[SIDX(ST_Z + j)];
            st[SIDX(ST_C + i)] += zi * u;
          }
        }
        RING_SHIFT(ur, u);
        RING_SHIFT(er, e);
      });
      if (solve_here) {
        float tr = 0.0f;
        for (int i = 0; i < K; ++i) tr += st[SIDX(ST_A + i * 8 + i)];
        const float lam = RIDGE * fmaxf(1.0f, tr / (float)K);
        for (int i = 0; i < K; ++i) {
          st[SIDX(ST_A + i * 8 + i)] += lam;
          for (int j = i + 1; j < K; ++j)
            st[SIDX(ST_A + j * 8 + i)] = st[SIDX(ST_A + i * 8 + j)];
        }
        chol_solve(st, lane, K);
        float sp = 0.0f, sq = 0.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i) { PHI(i) = 0.0f; THETA(i) = 0.0f; }
        for (int i = 0; i < p; ++i) PHI(i) = st[SIDX(ST_C + i)];
        for (int j = 0; j < q; ++j) THETA(j) = st[SIDX(ST_C + p + j)];
#pragma unroll
        for (int i = 0; i < 4; ++i) sp += fabsf(PHI(i));
#pragma unroll
        for (int j = 0; j < 4; ++j) sq += fabsf(THETA(j));
        if (sp > SHRINK) {
          const float s = SHRINK / sp;
#pragma unroll
          for (int i = 0; i < 4; ++i) PHI(i) *= s;
        }
        if (sq > SHRINK) {
          const float s = SHRINK / sq;
#pragma unroll
          for (int j = 0; j < 4; ++j) THETA(j) *= s;
        }
      }
    }
    // final innovation pass under the final coefs (leaves the rings at
    // the end of the series for stage 5 / the fitted-value writer)
    if (any_q) {
      load_arma(st, lane, phr, thr);
      rings_clear(ur, er);
      stream_u([&](int, float u) {
        const float e = innovation(u, phr, thr, ur, er);
        RING_SHIFT(ur, u);
        RING_SHIFT(er, e);
      });
    }
  }

  float chk = ur[0] + er[0] + wm;
#pragma unroll
  for (int i = 0; i < 4; ++i) chk += PHI(i) + THETA(i);
  for (int k = 0; k < KX; ++k) chk += BETA(k);
  *ok_out = isfinite(chk);
  return wm;
}

// Candidate evaluation: every group fits every order of the list on rows
// 0..S-1 and is scored on the H = T - S rows after them.
extern "C" __global__ __launch_bounds__(WAVE) void groupfit_eval_kernel(
    const float* __restrict__ yT,
    const float* __restrict__ xc0, const float* __restrict__ xc1,
    const float* __restrict__ xc2,
    const float* __restrict__ pj0, const float* __restrict__ pj1,
    const float* __restrict__ pj2,
    const int* __restrict__ orders, float* __restrict__ mse,
    unsigned char* __restrict__ status,
    const float* __restrict__ b0, const float* __restrict__ b1,
    const float* __restrict__ b2,
    const float* __restrict__ w0, const float* __restrict__ w1,
    const float* __restrict__ w2,
    int T, long long G, int S, int C, int KX) {
  __shared__ float st[NSTATE * WAVE];
  const int lane = threadIdx.x;
  const long long g = (long long)blockIdx.x * WAVE + lane;
  const bool active = g < G;
  const long long gg = active ? g : (G - 1);
  const int H = T - S;
  const LdsBeta beta{st, lane};
  float ur[8], er[8], ph[4], th[4];

  for (int c = 0; c < C; ++c) {
    const Order o = load_order(orders + c * 3);
    const int p = o.p, d = o.d, q = o.q;
    const float* xc = PICK_D(d, xc);
    const int n = S - d;
    bool ok;
    const float wm = fit_lane(
        yT, xc, PICK_D(d, pj), st, lane, gg, G, S, KX,
        p, d, q, &ok, ur, er, PICK_D(d, b),
        PICK_D(d, w));

    // ---- stage 5: validation forecast + MSE (rings hold u/e at n-1-j)
    load_arma(st, lane, ph, th);
    float yl1 = yT[(long long)(S - 1) * G + gg];
    float yl2 = (S - 2 >= 0) ? yT[(long long)(S - 2) * G + gg] : 0.f;
    float sse = 0.0f;
    for (int h = 0; h < H; ++h) {
      const float w_pred = forecast_step(xc, n + h, beta, KX, wm, ph, th, ur,
                                         er);
      // d = 1 adds to a running y here, while the forecast kernel sums
      // w_pred first; merging the two would change the MSE bits
      float y_pred;
      if (d == 0) y_pred = w_pred;
      else if (d == 1) { y_pred = yl1 + w_pred; yl2 = yl1; yl1 = y_pred; }
      else { y_pred = w_pred + 2.0f * yl1 - yl2; yl2 = yl1; yl1 = y_pred; }
      const float yv = yT[(long long)(S + h) * G + gg];
      const float err = yv - y_pred;
      sse += err * err;
    }
    const float m = sse / (float)H;
    if (active) {
      const bool fin = ok && isfinite(m);
      mse[(long long)c * G + g] = fin ? m : INFINITY;
      status[(long long)c * G + g] = fin ? 1 : 0;
    }
  }
}

// Final fit: per-group chosen order (may differ per lane — the passes
// are wave-voted, per-lane work predicated) on the whole series. Writes
// one-step-ahead fitted values, the coefficient vector and status.
extern "C" __global__ __launch_bounds__(WAVE) void groupfit_final_kernel(
    const float* __restrict__ yT,
    const float* __restrict__ xc0, const float* __restrict__ xc1,
    const float* __restrict__ xc2,
    const float* __restrict__ pj0, const float* __restrict__ pj1,
    const float* __restrict__ pj2,
    const int* __restrict__ best_order, float* __restrict__ fitted,
    float* __restrict__ params, unsigned char* __restrict__ status,
    const float* __restrict__ b0, const float* __restrict__ b1,
    const float* __restrict__ b2,
    const float* __restrict__ w0, const float* __restrict__ w1,
    const float* __restrict__ w2,
    int T, long long G, int KX) {
  __shared__ float st[NSTATE * WAVE];
  const int lane = threadIdx.x;
  const long long g = (long long)blockIdx.x * WAVE + lane;
  const bool active = g < G;
  const long long gg = active ? g : (G - 1);
  const Order o = load_order(best_order + gg * 3);
  const int p = o.p, d = o.d, q = o.q;
  const float* xc = PICK_D(d, xc);
  float ur[8], er[8], ph[4], th[4];

  bool ok;
  const float wm = fit_lane(
      yT, xc, PICK_D(d, pj), st, lane, gg, G, T, KX,
      p, d, q, &ok, ur, er, PICK_D(d, b),
      PICK_D(d, w));

  // Fitted-value pass. Not through stream_w: the d warm-up steps write
  // y itself, and the integration needs the y ring from before the step.
  {
    const LdsBeta beta{st, lane};
    load_arma(st, lane, ph, th);
    rings_clear(ur, er);
    float y0 = 0.f, y1 = 0.f;
    for (int t = 0; t < T; ++t) {
      const float yv = yT[(long long)t * G + gg];
      const float yl1 = y0, yl2 = y1;
      const float w = diff_step(d, yv, y0, y1);
      float out;
      if (t < d) {
        out = yv;
      } else {
        const float regx = reg_term(xc, t - d, beta, KX);
        float acc;
        insample_step(w, wm, regx, ph, th, ur, er, acc);
        const float what = wm + regx + acc;
        if (d == 0) out = what;
        else if (d == 1) out = yl1 + what;
        else out = 2.0f * yl1 - yl2 + what;
      }
      if (active) fitted[(long long)t * G + g] = out;
    }
  }

  if (active) {
    float* pp = params + g * (1 + KX + 8);
    pp[0] = wm;
    for (int k = 0; k < KX; ++k) pp[1 + k] = BETA(k);
    for (int i = 0; i < 4; ++i) {
      pp[1 + KX + i] = PHI(i);
      pp[1 + KX + 4 + i] = THETA(i);
    }
    status[g] = ok ? 1 : 0;
  }
}

// Out-of-sample forecast from STORED coefficients: no fitting and no LDS
// state block. wm, beta, phi, theta come from `params` into registers; one
// streaming pass of insample_step rebuilds the end-of-series u/e rings and
// accumulates
//   sigma2 = 1/(n-m) sum_{td>=m} e_td^2,   m = max(p,q);
// then H forecast_steps, integrated to y-units, next to the psi-weight
// recursion of the ARIMA(p,d,q) process
//   1 - sum a_k B^k = (1 - sum phi_i B^i)(1-B)^d        (p + d <= 6)
//   psi_0 = 1,  psi_j = theta_j [j<=q] + sum_k a_k psi_{j-k}
//   se_h  = sqrt(sigma2 * sum_{j<=h} psi_j^2).
// Orders are per lane; clamped, a lane always has n - m >= T - 6 residuals
// and reads inside xc{d}.
extern "C" __global__ __launch_bounds__(WAVE) void groupfit_forecast_kernel(
    const float* __restrict__ yT,
    const float* __restrict__ xc0, const float* __restrict__ xc1,
    const float* __restrict__ xc2,
    const int* __restrict__ best_order, const float* __restrict__ params,
    float* __restrict__ forecast, float* __restrict__ forecast_se,
    float* __restrict__ sigma2v, unsigned char* __restrict__ status,
    int T, long long G, int KX, int H) {
  const int lane = threadIdx.x;
  const long long g = (long long)blockIdx.x * WAVE + lane;
  const bool active = g < G;
  const long long gg = active ? g : (G - 1);
  const Order o = load_order(best_order + gg * 3);
  const int p = o.p, d = o.d, q = o.q;
  const float* xc = PICK_D(d, xc);
  const int n = T - d;
  const int m = max(p, q);

  const float* pp = params + gg * (1 + KX + 8);
  const float wm = pp[0];
  float beta[MAXK], ph[4], th[4];
#pragma unroll
  for (int k = 0; k < MAXK; ++k) beta[k] = (k < KX) ? pp[1 + k] : 0.0f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ph[i] = pp[1 + KX + i];
    th[i] = pp[1 + KX + 4 + i];
  }

  // ---- streaming pass: end-of-series rings + residual sum of squares.
  // Not through stream_w: the y load of step t+1 is issued before the
  // recursion of step t.
  float ur[8], er[8];
  rings_clear(ur, er);
  float y0 = 0.0f, y1 = 0.0f, sse = 0.0f;
  float ynext = yT[gg];
  for (int t = 0; t < T; ++t) {
    const float yv = ynext;
    if (t + 1 < T) ynext = yT[(long long)(t + 1) * G + gg];
    const float w = diff_step(d, yv, y0, y1);
    if (t >= d) {
      const int td = t - d;
      const float regx = reg_term(xc, td, beta, KX);
      float acc;
      const float e = insample_step(w, wm, regx, ph, th, ur, er, acc);
      if (td >= m) sse += e * e;
    }
  }
  const float sigma2 = sse / (float)(n - m);

  // ---- a_k = -c_k, c = (1 - sum phi_i B^i)(1-B)^d, by polynomial product
  float c[7];
  c[0] = 1.0f;
#pragma unroll
  for (int i = 0; i < 4; ++i) c[1 + i] = -ph[i];
  c[5] = 0.0f; c[6] = 0.0f;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    if (r < d) {
#pragma unroll
      for (int k = 6; k > 0; --k) c[k] = c[k] - c[k - 1];
    }
  }

  // ---- H steps: forecast recursion + psi recursion. pr[j] = psi_{h-1-j};
  // tq is theta shifted so that tq[0] is the theta term of the next psi.
  float pr[8], tq[4];
#pragma unroll
  for (int j = 0; j < 8; ++j) pr[j] = 0.0f;
#pragma unroll
  for (int i = 0; i < 4; ++i) tq[i] = th[i];
  float psi = 1.0f, cum = 0.0f;
  const float ylast = y0;        // y_{T-1}
  float yl1 = y0, yl2 = y1;      // y_{T-1}, y_{T-2}
  float wsum = 0.0f;
  bool fin = isfinite(sigma2);
  for (int h = 0; h < H; ++h) {
    const float w_pred = forecast_step(xc, n + h, beta, KX, wm, ph, th, ur,
                                       er);
    // d = 1 sums the small w_pred first and adds y_{T-1} once, as the
    // oracle does: one rounding at the size of y, not one per step
    float y_pred;
    if (d == 0) {
      y_pred = w_pred;
    } else if (d == 1) {
      wsum += w_pred;
      y_pred = ylast + wsum;
    } else {
      y_pred = w_pred + 2.0f * yl1 - yl2;
      yl2 = yl1; yl1 = y_pred;
    }

    cum += psi * psi;            // psi = psi_h here
    const float se = sqrtf(sigma2 * cum);
    RING_SHIFT(pr, psi);
    psi = tq[0];
#pragma unroll
    for (int k = 0; k < 6; ++k) psi -= c[1 + k] * pr[k];
    tq[0] = tq[1]; tq[1] = tq[2]; tq[2] = tq[3]; tq[3] = 0.0f;

    fin = fin && isfinite(y_pred) && isfinite(se);
    if (active) {
      forecast[(long long)h * G + g] = y_pred;
      forecast_se[(long long)h * G + g] = se;
    }
  }
  if (active) {
    sigma2v[g] = sigma2;
    status[g] = fin ? 1 : 0;
  }
}

// One wave of 64 groups per block. The kernels take their operands one by
// one so that the pointers are __restrict__ kernel arguments: read through
// a struct they lose that, and the uniform loads of the orders and the
// design rows stop being scalar loads.
#define WAVE_GRID(G) dim3((int)(((G) + WAVE - 1) / WAVE)), dim3(WAVE), 0

extern "C" void launch_groupfit_eval(const GroupfitEvalArgs& a,
                                     hipStream_t stream) {
  hipLaunchKernelGGL(groupfit_eval_kernel, WAVE_GRID(a.G), stream, a.yT,
                     a.xc0, a.xc1, a.xc2, a.pj0, a.pj1, a.pj2, a.orders,
                     a.mse, a.status, a.b0, a.b1, a.b2, a.w0, a.w1, a.w2,
                     a.T, a.G, a.S, a.C, a.KX);
}

extern "C" void launch_groupfit_final(const GroupfitFinalArgs& a,
                                      hipStream_t stream) {
  hipLaunchKernelGGL(groupfit_final_kernel, WAVE_GRID(a.G), stream, a.yT,
                     a.xc0, a.xc1, a.xc2, a.pj0, a.pj1, a.pj2, a.best_order,
                     a.fitted, a.params, a.status, a.b0, a.b1, a.b2, a.w0,
                     a.w1, a.w2, a.T, a.G, a.KX);
}

extern "C" void launch_groupfit_forecast(const GroupfitForecastArgs& a,
                                         hipStream_t stream) {
  hipLaunchKernelGGL(groupfit_forecast_kernel, WAVE_GRID(a.G), stream, a.yT,
                     a.xc0, a.xc1, a.xc2, a.best_order, a.params,
                     a.forecast, a.forecast_se, a.sigma2, a.status, a.T,
                     a.G, a.KX, a.H);
}
