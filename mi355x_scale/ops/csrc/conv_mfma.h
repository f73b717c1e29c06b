// What the MFMA conv kernels share (conv1x1.hip, conv3x3.hip,
// conv3x3wrw.hip, conv3x3s2.hip): operand types, the transposed LDS fragment
// read with its panel swizzle, and the padded-flat geometry of the 3x3
// kernels, stride 1 and stride 2.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

typedef __bf16 bf16;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;

// one MFMA operand (8 K values per lane) from two transposed block reads
__device__ __forceinline__ bf16x8 tr_frag(const bf16* p0, const bf16* p1) {
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p0);
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p1);
  const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, v);
}

// element offset of 16-byte chunk ``ch`` of row ``row`` in a [rows][64]
// panel that transposed reads take rows out of (bank reasoning in
// conv1x1.hip); the term depends on row & 15 only
__device__ __forceinline__ int wswz(int row, int ch) {
  const int f = (((row & 3) ^ ((row >> 3) & 1)) << 1) | ((row >> 2) & 1);
  return row * 64 + ((ch ^ f) << 3);
}

// Padded-flat coordinates of a 3x3 / stride 1 / pad 1 conv: the map is seen
// as a virtual zero-bordered [N][H+2][W+2] with flat index q. The padded
// map's row length and image size, floor(2^32 / d) for both, and the
// virtual pixel count Q = N*(H+2)*(W+2) (below 2^31).
struct C3Geo {
  int H, W, Wp, HpWp, Q;
  unsigned rWp, rHpWp;
};

// q = m / d, m -= q * d: m * floor(2^32/d) / 2^32 lies in (m/d - 1, m/d]
__device__ __forceinline__ unsigned c3_divmod(unsigned& m, unsigned d,
                                              unsigned rd) {
  unsigned q = __umulhi(m, rd);
  m -= q * d;
  if (m >= d) {
    m -= d;
    ++q;
  }
  return q;
}

// virtual pixel q (any value) -> its row in the real map, or -1 on the
// zero border and outside [0, Q)
__device__ __forceinline__ int c3_pixel(long long q, const C3Geo& g) {
  if (q < 0 || q >= g.Q) return -1;
  unsigned m = (unsigned)q;
  const unsigned n = c3_divmod(m, (unsigned)g.HpWp, g.rHpWp);
  const unsigned hp = c3_divmod(m, (unsigned)g.Wp, g.rWp);  // m is now wp
  if (hp - 1u >= (unsigned)g.H || m - 1u >= (unsigned)g.W) return -1;
  return (int)((n * g.H + hp - 1u) * g.W + m - 1u);
}

// floor(2^32 / d), saturated for d = 1: the multiplier c3_divmod takes
static inline unsigned c3_recip(long long d) {
  const long long r = (1LL << 32) / d;
  return r > 0xffffffffLL ? 0xffffffffu : (unsigned)r;
}

static inline C3Geo c3_geo(int N, int H, int W) {
  const long long hpwp = (long long)(H + 2) * (W + 2);
  return {H, W, W + 2, (int)hpwp, (int)(N * hpwp),
          c3_recip(W + 2), c3_recip(hpwp)};
}

// Padded-flat coordinates of a 3x3 / stride 2 / pad 1 conv: the OUTPUT grid
// [N][Ho][Wo], Ho = (H+1)/2, Wo = (W+1)/2, is seen as a virtual map
// [N][Ho+1][Wo+1] with one leading zero row and column per image, flat index
// q = (n*(Ho+1) + ho+1)*Wp + wo+1, Wp = Wo+1. The four parity planes of the
// input, P[ph][pw][i][j] = X[2i+ph][2j+pw], lie on the same grid. Row length
// and image size of the virtual map, floor(2^32 / d) for both, and the
// virtual pixel count Q = N*(Ho+1)*Wp (below 2^31).
struct C3S2Geo {
  int H, W, Ho, Wo, Wp, HpWp, Q;
  unsigned rWp, rHpWp;
};

// virtual pixel q (any value) -> its cell (n, i, j) of the output grid (and
// of every parity plane); false on the zero border and outside [0, Q)
__device__ __forceinline__ bool c3s2_cell(long long q, const C3S2Geo& g,
                                          int& n, int& i, int& j) {
  if (q < 0 || q >= g.Q) return false;
  unsigned m = (unsigned)q;
  n = (int)c3_divmod(m, (unsigned)g.HpWp, g.rHpWp);
  i = (int)c3_divmod(m, (unsigned)g.Wp, g.rWp) - 1;  // m is now wo + 1
  j = (int)m - 1;
  return i >= 0 && j >= 0;
}

static inline C3S2Geo c3s2_geo(int N, int H, int W) {
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  const long long hpwp = (long long)(Ho + 1) * (Wo + 1);
  return {H, W, Ho, Wo, Wo + 1, (int)hpwp, (int)(N * hpwp),
          c3_recip(Wo + 1), c3_recip(hpwp)};
}
