// Batched Holt-Winters (ExponentialSmoothing) fit for gfx950 (MI355X).
//
// The estimator is the fixed-schedule search of forecast/holtwinters.py
// (numpy oracle: forecast/batched_hw.py): a coarse grid over
// (alpha, beta, gamma, phi), two 3x3 (alpha, beta) refinement rounds, one
// final pass at the winner. Every candidate is one T-step recursion with
// a tiny per-series state, so the layout is groupfit.hip's: ONE GROUP PER
// LANE, 64 groups per wave, TIME-MAJOR [T][G] series so each per-timestep
// access is one coalesced 64-lane load; tail lanes are clamped to G-1 on
// load and masked on store.
//
// hwfit_search: a block owns 64 groups and runs NW waves; wave w scores
//   candidates w, w+NW, ... of the SAME 64 groups, then the waves meet in
//   LDS for an argmin (lowest SSE, lowest candidate index among equals —
//   the scalar class's "first strict minimum"). The refinement rounds run
//   the same way over their 9 candidates. One call site evaluates every
//   candidate of every phase, so a candidate's arithmetic depends on its
//   parameters alone, never on the wave or phase that scored it.
//     - level / trend / SSE live in registers;
//     - the seasonal state is indexed by t % m at run time, so it lives in
//       LDS (m x 64 floats per wave), never in a register array;
//     - the block's [T][64] y slab is staged in LDS once when it fits
//       (40 KB at T = 157) and re-read per candidate from there; longer
//       series stream from global (L2-resident after the first pass).
//   A lane's recursion is one dependent chain; y_{t+1} and the next
//   seasonal index are fetched before step t's arithmetic so only the
//   arithmetic is on the chain. The first m steps read the INITIAL
//   seasonal indices, which are a function of y_t and the init state, so
//   they are computed in flight and the LDS state needs no per-candidate
//   reset.
// hwfit_final: one wave per 64 groups, one pass at the given parameters,
//   in double: fitted values, end state, SSE, H-step forecast. Also the
//   whole job when the caller supplies the parameters.

#include <hip/hip_runtime.h>
#include <math.h>
#include <type_traits>

// Every fused multiply-add below is written out as fmaf; the compiler
// may not form others. A candidate's SSE is then the same bits wherever
// the evaluation is inlined, which the argmin's tie rules rely on (the
// refinement's centre candidate must tie with the incumbent, not beat it).
#pragma clang fp contract(off)

#define WAVE 64
#define HW_MAXM 64           // seasonal_periods cap (16 KB of LDS per wave)
#define HW_MAX_WAVES 16
#define HW_TINY 1e-9
#define HW_SENT 0x7fffffff
#define HW_LDS_BUDGET (160 * 1024)
#define HW_SLAB_MAX (80 * 1024)   // stage y only if it leaves half the LDS

// y_t of this lane's group: LDS slab (stride 64) or global (stride G).
struct YLds {
  const float* p;
  __device__ __forceinline__ float operator()(int t) const {
    return p[t * WAVE];
  }
};
struct YGlobal {
  const float* p;
  long long G;
  __device__ __forceinline__ float operator()(int t) const {
    return p[(long long)t * G];
  }
};

__device__ __forceinline__ float hw_fma(float a, float b, float c) {
  return fmaf(a, b, c);
}
__device__ __forceinline__ double hw_fma(double a, double b, double c) {
  return fma(a, b, c);
}
__device__ __forceinline__ float hw_max(float a, float b) {
  return fmaxf(a, b);
}
__device__ __forceinline__ double hw_max(double a, double b) {
  return fmax(a, b);
}

// The recursion is written once over the arithmetic type F: float in the
// search (the hot path), double in the final pass (1/1000 of the work;
// see hwfit_final_kernel).
template <class F>
struct HwInit {
  F lvl0, b0, s0;
  bool full;   // n >= 2m: first-season init; else first-value fallback
};

template <int SEAS, bool TREND, class F, class Y>
__device__ __forceinline__ HwInit<F> hw_init(const Y& y, int T, int m) {
  HwInit<F> in;
  in.full = SEAS != 0 && T >= 2 * m;
  if (in.full) {
    F a = 0, c = 0;
    for (int j = 0; j < m; ++j) { a += (F)y(j); c += (F)y(m + j); }
    in.s0 = a / (F)m;
    in.lvl0 = in.s0;
    in.b0 = TREND ? (c / (F)m - in.s0) / (F)m : (F)0;
  } else {
    in.s0 = 0;
    in.lvl0 = (F)y(0);
    in.b0 = TREND ? (F)y(1) - (F)y(0) : (F)0;
  }
  return in;
}

// initial seasonal index j (detrended first season, or the neutral value)
template <int SEAS, class F>
__device__ __forceinline__ F hw_seas0(F yj, int j, int m,
                                      const HwInit<F>& in) {
  if (!in.full) return SEAS == 2 ? (F)1 : (F)0;
  const F base = in.s0 + in.b0 * ((F)j - (F)0.5 * (F)(m - 1));
  return SEAS == 2 ? yj / hw_max(base, (F)HW_TINY) : yj - base;
}

// One recursion step. Updates lvl/b/sse, sets yhat, returns the new
// seasonal index for slot t % m.
template <int SEAS, bool TREND, class F>
__device__ __forceinline__ F hw_step(F yt, F si, F alpha, F beta, F gamma,
                                     F phi, F& lvl, F& b, F& sse, F& yhat) {
  const F one = 1;
  const F base = hw_fma(phi, b, lvl);
  yhat = SEAS == 2 ? base * si : base + si;
  const F err = yt - yhat;
  sse = hw_fma(err, err, sse);
  const F des = SEAS == 2 ? yt / hw_max(si, (F)HW_TINY) : yt - si;
  const F nl = hw_fma(alpha, des, (one - alpha) * base);
  if (TREND) b = hw_fma(beta, nl - lvl, (one - beta) * phi * b);
  lvl = nl;
  if (SEAS == 2)
    return hw_fma(gamma, yt / hw_max(nl, (F)HW_TINY), (one - gamma) * si);
  if (SEAS == 1) return hw_fma(gamma, yt - nl, (one - gamma) * si);
  return 0;
}

// SSE of one candidate. seas points at this lane's column of the wave's
// LDS seasonal state (slot j at seas[j * 64]); unused when SEAS == 0.
template <int SEAS, bool TREND, class Y>
__device__ __forceinline__ float hw_eval(const Y& y, float* seas, int T,
                                         int m, const HwInit<float>& in,
                                         float alpha, float beta,
                                         float gamma, float phi) {
  float lvl = in.lvl0, b = in.b0, sse = 0.0f, yhat;
  const int T0 = SEAS ? min(m, T) : T;
  float yn = y(0);
  for (int t = 0; t < T0; ++t) {
    const float yt = yn;
    yn = y(min(t + 1, T - 1));
    const float si = SEAS ? hw_seas0<SEAS, float>(yt, t, m, in) : 0.0f;
    const float sn = hw_step<SEAS, TREND, float>(yt, si, alpha, beta, gamma,
                                                 phi, lvl, b, sse, yhat);
    if (SEAS) seas[t * WAVE] = sn;
  }
  if (SEAS && T > m) {
    int j = 0;
    float s_next = seas[0];
    for (int t = m; t < T; ++t) {
      const float yt = yn;
      yn = y(min(t + 1, T - 1));
      const float si = s_next;
      const int jn = (j + 1 == m) ? 0 : j + 1;
      s_next = seas[jn * WAVE];   // m >= 2: slot jn != slot j
      const float sn = hw_step<SEAS, TREND, float>(yt, si, alpha, beta, gamma,
                                                   phi, lvl, b, sse, yhat);
      seas[j * WAVE] = sn;
      j = jn;
    }
  }
  return sse;
}

__device__ __forceinline__ float hw_clip(float v, float lo, float hi) {
  return fminf(fmaxf(v, lo), hi);
}

template <int SEAS, bool TREND, bool STAGED>
__global__ __launch_bounds__(HW_MAX_WAVES * WAVE) void hwfit_search_kernel(
    const float* __restrict__ yT,       // [T][G]
    const float* __restrict__ table,    // [C][4] product order
    float* __restrict__ params,         // [G][4]
    float* __restrict__ sse_out,        // [G]
    unsigned char* __restrict__ statusv,  // [G]
    int T, long long G, int C, int m) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nw = blockDim.x >> 6;
  const long long g0 = (long long)blockIdx.x * WAVE;
  const long long g = g0 + lane;
  const bool active = g < G;
  const long long gg = active ? g : (G - 1);

  // LDS: [y slab T*64][seasonal state nw*m*64][argmin sse nw*64][idx nw*64]
  const int slab_n = STAGED ? T * WAVE : 0;
  float* seas = lds + slab_n + (SEAS ? wave * m * WAVE : 0) + lane;
  float* red_s = lds + slab_n + (SEAS ? nw * m * WAVE : 0);
  int* red_c = reinterpret_cast<int*>(red_s + nw * WAVE);

  if (STAGED) {
    for (int i = tid; i < T * WAVE; i += blockDim.x) {
      const int t = i >> 6;
      long long gl = g0 + (i & (WAVE - 1));
      if (gl > G - 1) gl = G - 1;
      lds[i] = yT[(long long)t * G + gl];
    }
    __syncthreads();
  }
  typename std::conditional<STAGED, YLds, YGlobal>::type y;
  if constexpr (STAGED) {
    y.p = lds + lane;
  } else {
    y.p = yT + gg;
    y.G = G;
  }
  const HwInit<float> in = hw_init<SEAS, TREND, float>(y, T, m);

  float best_s = INFINITY;
  float ca = 0.0f, cb = 0.0f, cg = 0.0f, cp = 1.0f;
  // phase 0: the grid; phases 1-2: the 3x3 neighbourhood of (ca, cb)
  for (int phase = 0; phase < 3; ++phase) {
    const int n = phase == 0 ? C : 9;
    float ls = INFINITY;
    int lc = HW_SENT;
    for (int c = wave; c < n; c += nw) {
      float a, b, gm, p;
      if (phase == 0) {
        a = table[c * 4 + 0]; b = table[c * 4 + 1];
        gm = table[c * 4 + 2]; p = table[c * 4 + 3];
      } else {
        a = hw_clip(ca + (float)(c / 3 - 1) * 0.05f, 0.01f, 0.99f);
        b = hw_clip(cb + (float)(c % 3 - 1) * 0.05f, 0.0f, 0.99f);
        gm = cg; p = cp;
      }
      float s = hw_eval<SEAS, TREND>(y, seas, T, m, in, a, b, gm, p);
      if (!isfinite(s)) s = INFINITY;
      if (s < ls) { ls = s; lc = c; }
    }
    red_s[wave * WAVE + lane] = ls;
    red_c[wave * WAVE + lane] = lc;
    __syncthreads();
    float bs = INFINITY;
    int bc = HW_SENT;
    for (int w = 0; w < nw; ++w) {
      const float s = red_s[w * WAVE + lane];
      const int c = red_c[w * WAVE + lane];
      if (s < bs || (s == bs && c < bc)) { bs = s; bc = c; }
    }
    __syncthreads();
    if (phase == 0) {
      if (bc == HW_SENT) bc = 0;   // no finite candidate: keep the first
      best_s = bs;
      ca = table[bc * 4 + 0]; cb = table[bc * 4 + 1];
      cg = table[bc * 4 + 2]; cp = table[bc * 4 + 3];
    } else if (bs < best_s) {      // the incumbent wins ties
      best_s = bs;
      ca = hw_clip(ca + (float)(bc / 3 - 1) * 0.05f, 0.01f, 0.99f);
      cb = hw_clip(cb + (float)(bc % 3 - 1) * 0.05f, 0.0f, 0.99f);
    }
  }

  if (active && wave == 0) {
    const bool ok = isfinite(best_s);
    const float nanv = __builtin_nanf("");
    float* pp = params + g * 4;
    pp[0] = ok ? ca : nanv; pp[1] = ok ? cb : nanv;
    pp[2] = ok ? cg : nanv; pp[3] = ok ? cp : nanv;
    sse_out[g] = ok ? best_s : nanv;
    statusv[g] = ok ? 1 : 0;
  }
}

template <int SEAS, bool TREND>
__global__ __launch_bounds__(WAVE) void hwfit_final_kernel(
    const float* __restrict__ yT,       // [T][G]
    const float* __restrict__ params,   // [G][4]
    float* __restrict__ fitted,         // [T][G]
    float* __restrict__ forecast,       // [H][G]
    float* __restrict__ level,          // [G]
    float* __restrict__ trendv,         // [G]
    float* __restrict__ season,         // [m][G]
    float* __restrict__ sse_out,        // [G]
    unsigned char* __restrict__ statusv,  // [G]
    int T, long long G, int m, int H) {
  // The pass runs in double: the trend is a difference of consecutive
  // levels, and at f32 a level near 1000 carries 6e-5..1.2e-4 of rounding
  // that the difference keeps in full (beta near 1 on short series), more
  // than the state is specified to. One pass per group is ~0.1% of the
  // search's arithmetic. Inputs and outputs stay f32.
  extern __shared__ double seas_l[];   // [m][64], SEAS only
  const int lane = threadIdx.x;
  const long long g = (long long)blockIdx.x * WAVE + lane;
  const bool active = g < G;
  const long long gg = active ? g : (G - 1);
  double* seas = seas_l + lane;
  const double alpha = params[gg * 4 + 0], beta = params[gg * 4 + 1];
  const double gamma = params[gg * 4 + 2], phi = params[gg * 4 + 3];
  YGlobal y;
  y.p = yT + gg;
  y.G = G;
  const HwInit<double> in = hw_init<SEAS, TREND, double>(y, T, m);
  if (SEAS)
    for (int j = 0; j < m; ++j)
      seas[j * WAVE] = hw_seas0<SEAS, double>(
          in.full ? (double)y(j) : 0.0, j, m, in);

  double lvl = in.lvl0, b = in.b0, sse = 0.0, yhat;
  int j = 0;
  for (int t = 0; t < T; ++t) {
    const double yt = y(t);
    const double si = SEAS ? seas[j * WAVE] : 0.0;
    const double sn = hw_step<SEAS, TREND, double>(
        yt, si, alpha, beta, gamma, phi, lvl, b, sse, yhat);
    if (active) fitted[(long long)t * G + g] = (float)yhat;
    if (SEAS) {
      seas[j * WAVE] = sn;
      j = (j + 1 == m) ? 0 : j + 1;
    }
  }
  const bool ok = isfinite((float)sse);
  const float nanv = __builtin_nanf("");
  if (__any(!ok)) {
    for (int t = 0; t < T; ++t)
      if (active && !ok) fitted[(long long)t * G + g] = nanv;
  }
  // forecast h = 1..H from the end state; slot (T + h - 1) % m
  double pw = 1.0;
  for (int h = 1; h <= H; ++h) {
    pw *= phi;
    const double damp = (phi == 1.0) ? phi * (double)h
                                     : phi * (1.0 - pw) / (1.0 - phi);
    const double base = TREND ? lvl + damp * b : lvl;
    const double si = SEAS ? seas[j * WAVE] : 0.0;
    const double out = SEAS == 2 ? base * si : base + si;
    if (active)
      forecast[(long long)(h - 1) * G + g] = ok ? (float)out : nanv;
    if (SEAS) j = (j + 1 == m) ? 0 : j + 1;
  }
  if (active) {
    level[g] = ok ? (float)lvl : nanv;
    trendv[g] = ok ? (float)b : nanv;
    for (int k = 0; k < m; ++k)
      season[(long long)k * G + g] =
          ok ? (SEAS ? (float)seas[k * WAVE] : 0.0f) : nanv;
    sse_out[g] = ok ? (float)sse : nanv;
    statusv[g] = ok ? 1 : 0;
  }
}

// Waves per block and LDS bytes of a search launch. The y slab is staged
// when it leaves at least half the LDS for seasonal state; the candidate
// list is then split over as many waves as fit (<= 16, <= C), or over
// waves_req when the caller asks for fewer.
static int hwfit_search_plan(int T, int m, int seas, int C, int waves_req,
                             int* staged_out, size_t* lds_out) {
  const size_t slab = (size_t)T * WAVE * sizeof(float);
  const bool staged = slab <= HW_SLAB_MAX;
  const size_t per_wave =
      (seas ? (size_t)m * WAVE * sizeof(float) : 0) + 2 * WAVE * sizeof(float);
  const size_t avail = HW_LDS_BUDGET - (staged ? slab : 0);
  int nw = (int)(avail / per_wave);
  if (nw > HW_MAX_WAVES) nw = HW_MAX_WAVES;
  if (nw > C) nw = C;
  if (waves_req > 0 && nw > waves_req) nw = waves_req;
  if (nw < 1) nw = 1;
  *staged_out = staged ? 1 : 0;
  *lds_out = (staged ? slab : 0) + (size_t)nw * per_wave;
  return nw;
}

template <int SEAS, bool TREND, bool STAGED>
static void hw_search_launch(const float* yT, const float* table,
                             float* params, float* sse,
                             unsigned char* statusv, int T, long long G,
                             int C, int m, int nw, size_t lds,
                             hipStream_t stream) {
  auto kern = hwfit_search_kernel<SEAS, TREND, STAGED>;
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              HW_LDS_BUDGET);
  const int blocks = (int)((G + WAVE - 1) / WAVE);
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(nw * WAVE), lds, stream, yT,
                     table, params, sse, statusv, T, G, C, m);
}

#define HW_SEARCH_CASE(S, TR)                                              \
  if (seas == S && (trend != 0) == TR) {                                   \
    if (staged)                                                            \
      hw_search_launch<S, TR, true>(yT, table, params, sse, statusv, T, G, \
                                    C, m, nw, lds, stream);                \
    else                                                                   \
      hw_search_launch<S, TR, false>(yT, table, params, sse, statusv, T,   \
                                     G, C, m, nw, lds, stream);            \
    return nw;                                                             \
  }

// Returns the waves per block used.
extern "C" int launch_hwfit_search(const float* yT, const float* table,
                                   float* params, float* sse,
                                   unsigned char* statusv, int T,
                                   long long G, int C, int trend, int seas,
                                   int m, int waves_req,
                                   hipStream_t stream) {
  if (T < 2 || G < 1 || C < 1 || m < 1 || m > HW_MAXM) return 0;
  int staged = 0;
  size_t lds = 0;
  const int nw = hwfit_search_plan(T, m, seas, C, waves_req, &staged, &lds);
  HW_SEARCH_CASE(0, false)
  HW_SEARCH_CASE(0, true)
  HW_SEARCH_CASE(1, false)
  HW_SEARCH_CASE(1, true)
  HW_SEARCH_CASE(2, false)
  HW_SEARCH_CASE(2, true)
  return 0;
}

#define HW_FINAL_CASE(S, TR)                                               \
  if (seas == S && (trend != 0) == TR) {                                   \
    hipLaunchKernelGGL((hwfit_final_kernel<S, TR>), dim3(blocks),          \
                       dim3(WAVE), S ? seas_bytes : 0, stream, yT, params, \
                       fitted, forecast, level, trendv, season, sse,       \
                       statusv, T, G, m, H);                               \
    return;                                                                \
  }

extern "C" void launch_hwfit_final(const float* yT, const float* params,
                                   float* fitted, float* forecast,
                                   float* level, float* trendv,
                                   float* season, float* sse,
                                   unsigned char* statusv, int T,
                                   long long G, int trend, int seas, int m,
                                   int H, hipStream_t stream) {
  if (T < 2 || G < 1 || H < 0 || m < 1 || m > HW_MAXM) return;
  const int blocks = (int)((G + WAVE - 1) / WAVE);
  const size_t seas_bytes = (size_t)m * WAVE * sizeof(double);
  HW_FINAL_CASE(0, false)
  HW_FINAL_CASE(0, true)
  HW_FINAL_CASE(1, false)
  HW_FINAL_CASE(1, true)
  HW_FINAL_CASE(2, false)
  HW_FINAL_CASE(2, true)
}
