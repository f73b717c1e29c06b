// What groupfit.hip shares with its neighbours: the launch operands, which
// bindings.cpp fills in, and the differencing step, with which
// mfma_project.hip builds the stage-1 panel.
#pragma once

#include <hip/hip_runtime.h>

// Operands common to the three kernels: yT is the time-major panel [T][G];
// xc{d} is the centered exog design of differencing order d, [rows-d][KX]
// with rows >= T (the forecast reads H rows past the history); pj{d} is
// its train pseudo-inverse [KX][S-d]; b{d} [KX][G] and w{d} [G] are the
// stage-1 results of the MFMA projection, or null to compute them in the
// kernel; orders are (p, d, q) i32 triples.
struct GroupfitEvalArgs {
  const float *yT, *xc0, *xc1, *xc2, *pj0, *pj1, *pj2;
  const int* orders;        // [C][3], every group fits every candidate
  float* mse;               // [C][G] validation MSE over rows S..T-1
  unsigned char* status;    // [C][G]
  const float *b0, *b1, *b2, *w0, *w1, *w2;
  int T;
  long long G;
  int S, C, KX;
};

struct GroupfitFinalArgs {
  const float *yT, *xc0, *xc1, *xc2, *pj0, *pj1, *pj2;
  const int* best_order;    // [G][3], one order per group
  float* fitted;            // [T][G] one-step-ahead, y-units
  float* params;            // [G][1+KX+8]: wm, beta[KX], phi[4], theta[4]
  unsigned char* status;    // [G]
  const float *b0, *b1, *b2, *w0, *w1, *w2;
  int T;
  long long G;
  int KX;
};

struct GroupfitForecastArgs {
  const float *yT, *xc0, *xc1, *xc2;   // xc{d}: [T+H-d][KX] stacked
  const int* best_order;    // [G][3]
  const float* params;      // [G][1+KX+8] as the final fit wrote them
  float *forecast, *forecast_se;       // [H][G]
  float* sigma2;            // [G]
  unsigned char* status;    // [G]
  int T;
  long long G;
  int KX, H;
};

extern "C" void launch_groupfit_eval(const GroupfitEvalArgs& a,
                                     hipStream_t stream);
extern "C" void launch_groupfit_final(const GroupfitFinalArgs& a,
                                      hipStream_t stream);
extern "C" void launch_groupfit_forecast(const GroupfitForecastArgs& a,
                                         hipStream_t stream);

#ifdef __HIPCC__
// w_t = diff^d(y)_t for d <= 2 from y_t and the ring y0 = y_{t-1},
// y1 = y_{t-2}, which it advances. Pre-sample y is zero, so w_t is only
// meaningful for t >= d.
__device__ __forceinline__ float diff_step(int d, float yv, float& y0,
                                           float& y1) {
  float w;
  if (d == 0) w = yv;
  else if (d == 1) w = yv - y0;
  else w = yv - 2.0f * y0 + y1;
  y1 = y0; y0 = yv;
  return w;
}
#endif
