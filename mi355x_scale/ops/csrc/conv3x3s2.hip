// Hand-written MFMA 3x3 / stride 2 / pad 1 convolution for gfx950, NHWC
// bf16: forward, forward with BatchNorm statistics in the epilogue, and
// data-grad. Cin, Cout multiples of 64 (they may differ), 1 <= W <= 128, any
// H and N. The weight-grad of these convs is not here.
//
// Why: every ResNet has three of them (layer{2,3,4}[0]), each followed by a
// BN whose reduce pass re-reads the map the conv just wrote. The stride-1
// kernel (conv3x3.hip) cannot serve them: its padded-flat trick needs a tap
// to be one constant offset from the output pixel, and at stride 2 it is
// not, in input coordinates.
//
//   Y[n,ho,wo,co] = sum_{kh,kw,ci} X[n,2ho+kh-1,2wo+kw-1,ci] * Wt[co,kh,kw,ci]
//
// Parity planes in padded-flat OUTPUT coordinates. With Ho = (H+1)/2, Wo =
// (W+1)/2, Wp = Wo+1, the input splits into four planes P[ph][pw][i][j] =
// X[2i+ph][2j+pw] (zero where 2i+ph >= H or 2j+pw >= W). Output (ho, wo)
// reads input row 2ho-1+kh: odd-plane row ho-1 (kh = 0), even-plane row ho
// (kh = 1), odd-plane row ho (kh = 2); columns alike. Seen on the virtual
// grid [N][Ho+1][Wp] with ONE leading zero row and column per image, q =
// (n*(Ho+1) + ho+1)*Wp + wo+1, every tap is a constant offset into exactly
// one plane:
//
//   plane (1,1): taps (0,0) (0,2) (2,0) (2,2), offsets -Wp-1, -Wp, -1, 0
//   plane (1,0): taps (0,1) (2,1),             offsets -Wp, 0
//   plane (0,1): taps (1,0) (1,2),             offsets -1, 0
//   plane (0,0): tap  (1,1),                   offset  0
//
// and crossing a row or an image edge lands on a zero border cell. The main
// loop has no division and no bounds test; every input pixel belongs to one
// plane, so a block fetches each 128-byte channel-chunk row of X once and
// gathers nothing per element. Useful MFMA share Ho*Wo / ((Ho+1)*(Wo+1)):
// 93 % at 28, 87 % at 14, 77 % at 7.
//
// Forward, conv3x3_s2_fwd_kernel<STATS>:
//   * work split of the stride-1 kernel: a block owns 128 consecutive q and
//     64 output channels, 256 threads, a wave 32 rows x 64 columns = 2 x 4
//     accumulator tiles, column tiles of one M-block adjacent in launch
//     order.
//   * K runs chunk-major (64 channels of Cin), plane-major in the order
//     above, tap-minor: nine steps per chunk.
//   * the unit of A staging is a plane band: virtual pixels q0-(Wp+1) ..
//     q0+127 of one plane and one chunk, 128 + Wo + 2 rows of 128 bytes,
//     global -> registers -> LDS with 16-byte accesses and the swizzle chunk
//     ^ (row & 7). Each staged row's cell (or "zero") is found ONCE per block
//     by two mul-hi divisions (C3S2Geo, conv_mfma.h); a plane only adds
//     ph*W + pw to the cell's pixel and tests two bits.
//   * TWO band buffers: the next plane's band (or the next chunk's first
//     plane) is loaded into registers before the first tap of the current
//     plane and stored into the other buffer after its last tap, in front of
//     that step's closing barrier. The other buffer was last read by the
//     previous plane, whose last step's barrier every wave has passed: no
//     extra barrier, and no step waits on a band.
//   * weight tiles are 64 co x 64 ci per tap from [Cout][3][3][Cin],
//     double-buffered, one barrier per step.
//   * LDS is sized from Wo at launch: 16 KB of weight tiles + two bands,
//     56,832 B at Wo = 28 (room for two blocks per CU), 53,248 at 14 and
//     51,456 at 7 (room for three), 66,048 at Wo = 64 (two; above 64 KB the
//     launch raises the kernel's dynamic LDS limit).
//   * epilogue, the stride-1 one: round to bf16, transpose through a
//     wave-private LDS tile, 16-byte stores of real pixels only. Statistics
//     are of the ROUNDED outputs with border rows forced to zero, lanes add
//     by shuffle, waves through LDS in a fixed order, one fp32 slot per
//     channel and M-block in [2*Cout][nblocks], nblocks = ceil(N*(Ho+1)*Wp /
//     128). No atomics: bit-reproducible.
//
// Data-grad, conv3x3_s2_dgrad_kernel: dX splits into the same four planes,
// and plane (ph, pw) of dX is a 4-, 2-, 2- or 1-tap convolution of dY over
// the same virtual grid with the offsets negated (+Wp+1, +Wp, +1, 0 ...).
// The plane is grid dimension y, the 4-tap plane first. A block stages ONE
// dY band (virtual pixels q0 .. q0+127+Wp+1) per 64-channel chunk of Cout,
// double-buffered across chunks in the same way, and runs its plane's taps
// against Wf[ci][8 - t][co], the repack conv3x3_wflip_kernel (conv3x3.hip)
// already writes. The epilogue sends row q to dX pixel (2i+ph, 2j+pw) where
// that lies inside H x W: every dX pixel is written exactly once by exactly
// one block, with no zero fill and no atomics.
//
// Both kernels share the operand staging, the MFMA step and the epilogue.
//
// Compiler resource usage (hipcc -O3, gfx950,
// -Rpass-analysis=kernel-resource-usage): conv3x3_s2_fwd_kernel 183 VGPRs
// with and without statistics, 2 waves per SIMD = 2 blocks per CU for every
// shape (the registers bind, not the LDS; three blocks would need 168);
// conv3x3_s2_dgrad_kernel 163 VGPRs, 3 waves per SIMD, so 3 blocks per CU
// where the LDS allows (Wo <= 19) and 2 above. LDS is dynamic, as above (at
// most 66,048 B). No VGPR spills; scratch is 0 for all three.
#include <hip/hip_runtime.h>
#include "conv_mfma.h"

#define S2_BM 128               // virtual pixels per block
#define S2_BN 64                // output channels per block
#define S2_BK 64                // channels per reduction chunk
#define S2_OTROW 72             // epilogue tile row stride (els): 144 B
#define S2_MAXU 7               // 32-row staging passes: ceil(194 / 32)

// element offset of 16-byte chunk ``ch`` of row ``row`` in a [rows][64] tile
__device__ __forceinline__ int s2_swz(int row, int ch) {
  return row * S2_BK + ((ch ^ (row & 7)) << 3);
}

// tap ``k`` of plane (ph, pw): an odd plane serves taps 0 and 2 of its axis,
// an even plane tap 1
__device__ __forceinline__ void s2_tap(int ph, int pw, int k, int& kh,
                                       int& kw) {
  kh = ph ? 2 * (k >> pw) : 1;
  kw = pw ? 2 * (k & 1) : 1;
}

// 64 rows x 64 K of the weight matrix [rows][9*KC] -> registers -> LDS tile
__device__ __forceinline__ void s2_w_load(bf16x8 (&rb)[2], const bf16* pb,
                                          int bstep, int kof) {
#pragma unroll
  for (int u = 0; u < 2; ++u)
    rb[u] = *reinterpret_cast<const bf16x8*>(pb + (long long)u * bstep + kof);
}
__device__ __forceinline__ void s2_w_store(const bf16x8 (&rb)[2], bf16* bs,
                                           int sto) {
#pragma unroll
  for (int u = 0; u < 2; ++u)
    *reinterpret_cast<bf16x8*>(bs + sto + u * 32 * S2_BK) = rb[u];
}

// staged band rows -> LDS; pix[u] == -2: beyond the band, nothing staged
__device__ __forceinline__ void s2_band_store(const bf16x8 (&ra)[S2_MAXU],
                                              const int (&pix)[S2_MAXU],
                                              bf16* as, int sto) {
#pragma unroll
  for (int u = 0; u < S2_MAXU; ++u)
    if (pix[u] != -2)
      *reinterpret_cast<bf16x8*>(as + sto + u * 32 * S2_BK) = ra[u];
}

// one K = 64 step of the wave's 32 x 64 tile: A rows r0, r0 + 16 of the band
// ``as``, B the weight tile ``bs``
__device__ __forceinline__ void s2_mfma_step(f32x4 (&acc)[2][4],
                                             const bf16* as, const bf16* bs,
                                             int r0, int kgrp, int bo0) {
  const int ao = r0 * S2_BK, asw = r0 & 7;  // r0 + 16: same & 7
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    const int fa = ((4 * kk + kgrp) ^ asw) << 3;
    bf16x8 af[2], bfr[4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
      af[m] = *reinterpret_cast<const bf16x8*>(as + ao + m * 16 * S2_BK + fa);
#pragma unroll
    for (int cc = 0; cc < 4; ++cc)
      bfr[cc] = *reinterpret_cast<const bf16x8*>(
          bs + cc * 16 * S2_BK + (kk ? bo0 ^ 32 : bo0));
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int cc = 0; cc < 4; ++cc)
        acc[m][cc] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            af[m], bfr[cc], acc[m][cc], 0, 0, 0);
  }
}

// Round, transpose through the wave's own LDS tile and store the rows whose
// ``opix`` (lanes l and l + 32 hold row l & 31 of the wave's 32) is a real
// pixel of ``Y`` [pixels][ldc]; STATS: this M-block's slot of the block's 64
// columns in partial [2*ldc][nmb]. The operand buffers must be free.
template <bool STATS>
__device__ __forceinline__ void s2_epilogue(const f32x4 (&acc)[2][4],
                                            int opix, bf16* smem,
                                            bf16* __restrict__ Y, int ldc,
                                            int n0, float* __restrict__ partial,
                                            int nmb, int mb) {
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, l16 = lane & 15, kgrp = lane >> 4;
  const unsigned real = (unsigned)__ballot(opix >= 0);  // bit r: row r is real

  // D col = lane&15, row = 4*(lane>>4)+r
  bf16* tw = smem + wave * 32 * S2_OTROW;
  float ssum[4] = {0.f, 0.f, 0.f, 0.f}, ssq[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = m * 16 + kgrp * 4 + r;
      const bool keep = (real >> row) & 1u;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        bf16 v = (bf16)acc[m][c][r];
        if (STATS) {
          // a border row's value is not an output: it adds nothing
          const float f = keep ? (float)v : 0.f;
          ssum[c] += f;
          ssq[c] += f * f;
        }
        tw[row * S2_OTROW + c * 16 + l16] = v;
      }
    }
  // the tile is wave-private and a wave's LDS operations complete in
  // order, so wave-scope ordering is all the hand-over needs
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int v = lane + t * 64;
    const int rl = v >> 3, j8 = (v & 7) * 8;
    const int p = __shfl(opix, rl, 64);
    const bf16x8 val =
        *reinterpret_cast<const bf16x8*>(tw + rl * S2_OTROW + j8);
    if (p >= 0)
      *reinterpret_cast<bf16x8*>(Y + (long long)p * ldc + n0 + j8) = val;
  }

  if (STATS) {
    // the four row groups of a wave, then the four waves (fixed order)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      ssum[c] += __shfl_xor(ssum[c], 16, 64);
      ssum[c] += __shfl_xor(ssum[c], 32, 64);
      ssq[c] += __shfl_xor(ssq[c], 16, 64);
      ssq[c] += __shfl_xor(ssq[c], 32, 64);
    }
    float* red = reinterpret_cast<float*>(smem + 4 * 32 * S2_OTROW);
    if (kgrp == 0) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        red[wave * 2 * S2_BN + c * 16 + l16] = ssum[c];
        red[wave * 2 * S2_BN + S2_BN + c * 16 + l16] = ssq[c];
      }
    }
    __syncthreads();
    if (tid < 2 * S2_BN) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) s += red[w * 2 * S2_BN + tid];
      const int ch = tid < S2_BN ? n0 + tid : ldc + n0 + tid - S2_BN;
      partial[(long long)ch * nmb + mb] = s;
    }
  }
}

// Y[pixel][Cout] over the virtual output pixels, Wt = [Cout][9][Cin]. grid =
// ceil(Q / 128) * (Cout / 64), column tiles fastest; dynamic LDS =
// conv3x3_s2_lds_bytes(Wo). phase_mask: 1 = global loads + LDS staging, 4 =
// MFMA, 2 = epilogue.
template <bool STATS>
__global__ __launch_bounds__(256, 2) void conv3x3_s2_fwd_kernel(
    const bf16* __restrict__ X, const bf16* __restrict__ Wt,
    bf16* __restrict__ Y,
    float* __restrict__ partial,  // [2*Cout][ceil(Q / 128)], STATS only
    int Cin, int Cout, int ntn, int phase_mask, const C3S2Geo g) {
  extern __shared__ __attribute__((aligned(16))) bf16 smem[];
  const int brows = S2_BM + g.Wp + 1;         // band rows
  bf16* const Bs = smem;                      // [2][64 co][64 ci]
  bf16* const As = smem + 2 * S2_BN * S2_BK;  // [2][brows][64 ci]
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int l16 = lane & 15;
  const int kgrp = lane >> 4;
  const int mb = blockIdx.x / ntn;
  const int nb = blockIdx.x - mb * ntn;
  const int q0 = mb * S2_BM, n0 = nb * S2_BN;
  const int nmb = gridDim.x / ntn;

  // staging: thread -> 16-byte chunk (tid & 7) of rows (tid >> 3) + 32u;
  // the swizzle term is the same for every u (32u is a multiple of 8)
  const int srow = tid >> 3, sch = tid & 7;
  const int sto = s2_swz(srow, sch);
  // band row b is virtual pixel q0 - (Wp+1) + b: the pixel (2i, 2j) of its
  // cell, -1 = a row of zeros in every plane, -2 = beyond the band. Bit u of
  // hm / wm: pixel row 2i+1 / column 2j+1 is inside the map.
  int pix[S2_MAXU];
  unsigned hm = 0, wm = 0;
#pragma unroll
  for (int u = 0; u < S2_MAXU; ++u) {
    const int b = srow + 32 * u;
    int n, i, j;
    pix[u] = -2;
    if (b < brows) {
      pix[u] = -1;
      if (c3s2_cell((long long)q0 - (g.Wp + 1) + b, g, n, i, j)) {
        pix[u] = (n * g.H + 2 * i) * g.W + 2 * j;
        hm |= (unsigned)(2 * i + 1 < g.H) << u;
        wm |= (unsigned)(2 * j + 1 < g.W) << u;
      }
    }
  }
  const bf16* const pa = X + sch * 8;
  const bf16* const pb = Wt + ((long long)n0 + srow) * 9 * Cin + sch * 8;
  const int bstep = 32 * 9 * Cin;  // 32 weight rows
  const bf16x8 zv = {(bf16)0.0f, (bf16)0.0f, (bf16)0.0f, (bf16)0.0f,
                     (bf16)0.0f, (bf16)0.0f, (bf16)0.0f, (bf16)0.0f};

  // operand addressing: B as the pointwise kernel; an A row moves with the
  // tap, so its swizzle term is taken per tap
  const int bo0 = l16 * S2_BK + ((kgrp ^ (l16 & 7)) << 3);  // K 0..31
  const int arow = wave * 32 + l16;

  f32x4 acc[2][4];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[m][c] = (f32x4)0.0f;

  bf16x8 ra[S2_MAXU], rb[2];

  // plane p = 0..3 is (1,1) (1,0) (0,1) (0,0)
#define S2_BAND_LOAD(p, cof)                                                \
  {                                                                         \
    const int ph_ = (p) < 2, pw_ = !((p) & 1);                              \
    _Pragma("unroll") for (int u = 0; u < S2_MAXU; ++u) {                   \
      const bool ok_ = pix[u] >= 0 && (!ph_ || ((hm >> u) & 1u)) &&         \
                       (!pw_ || ((wm >> u) & 1u));                          \
      ra[u] = ok_ ? *reinterpret_cast<const bf16x8*>(                       \
                        pa + (long long)(pix[u] + ph_ * g.W + pw_) * Cin +  \
                        (cof))                                              \
                  : zv;                                                     \
    }                                                                       \
  }

  if (phase_mask & 1) {
    S2_BAND_LOAD(0, 0)
    s2_w_load(rb, pb, bstep, 0);
    s2_band_store(ra, pix, As, sto);
    s2_w_store(rb, Bs, sto);
  }
  __syncthreads();

  const int nch = Cin / S2_BK;
#pragma unroll 1
  for (int c = 0; c < nch; ++c) {
    const bool nextc = c + 1 < nch;
#pragma unroll
    for (int s = 0; s < 9; ++s) {
      // step s of the chunk: plane p, its tap k; the step after it
      const int p = s < 4 ? 0 : (s - 2) / 2, k = s - (p ? 2 + 2 * p : 0);
      const int s1 = s < 8 ? s + 1 : 0;
      const int p1 = s1 < 4 ? 0 : (s1 - 2) / 2, k1 = s1 - (p1 ? 2 + 2 * p1 : 0);
      const bool first = k == 0, last = p1 != p;
      const int buf = (c + s) & 1;  // parity of step 9c + s
      const bool more = s < 8 || nextc;
      int kh, kw;
      if (more && (phase_mask & 1)) {
        s2_tap(p1 < 2, !(p1 & 1), k1, kh, kw);
        s2_w_load(rb, pb, bstep,
                  (3 * kh + kw) * Cin + (c + (s == 8)) * S2_BK);
      }
      // the band after this plane's: under this plane's MFMAs
      const bool nband = p < 3 || nextc;
      if (first && nband && (phase_mask & 1))
        S2_BAND_LOAD((p + 1) & 3, (c + (p == 3)) * S2_BK)
      if (phase_mask & 4) {
        s2_tap(p < 2, !(p & 1), k, kh, kw);
        s2_mfma_step(acc, As + (p & 1) * brows * S2_BK,
                     Bs + buf * S2_BN * S2_BK,
                     arow + (kh ? g.Wp : 0) + (kw ? 1 : 0), kgrp, bo0);
      }
      // the other band buffer was last read by plane p - 1, behind a barrier
      if (last && nband && (phase_mask & 1))
        s2_band_store(ra, pix, As + ((p + 1) & 1) * brows * S2_BK, sto);
      if (more && (phase_mask & 1))
        s2_w_store(rb, Bs + (buf ^ 1) * S2_BN * S2_BK, sto);
      __syncthreads();  // step s is read, step s+1 is in place
    }
  }
#undef S2_BAND_LOAD
  if (!(phase_mask & 2)) return;

  int n, i, j, opix = -1;
  if (c3s2_cell((long long)q0 + wave * 32 + (lane & 31), g, n, i, j))
    opix = (n * g.Ho + i) * g.Wo + j;
  s2_epilogue<STATS>(acc, opix, smem, Y, Cout, n0, partial, nmb, mb);
}

// dX[pixel][Cin] from dY [N][Ho][Wo][Cout] and Wf = [Cin][9][Cout] (rotated:
// Wf[ci][t][co] = Wt[co][8 - t][ci]). grid = (ceil(Q / 128) * (Cin / 64), 4):
// y is the dX plane, (1,1) (1,0) (0,1) (0,0); dynamic LDS as the forward.
__global__ __launch_bounds__(256, 2) void conv3x3_s2_dgrad_kernel(
    const bf16* __restrict__ dY, const bf16* __restrict__ Wf,
    bf16* __restrict__ dX, int Cin, int Cout, int ntn, int phase_mask,
    const C3S2Geo g) {
  extern __shared__ __attribute__((aligned(16))) bf16 smem[];
  const int ph = blockIdx.y < 2, pw = !(blockIdx.y & 1);
  if ((ph && g.H < 2) || (pw && g.W < 2)) return;  // an empty plane
  const int ntaps = (1 + ph) * (1 + pw);
  const int brows = S2_BM + g.Wp + 1;
  bf16* const Bs = smem;                      // [2][64 ci][64 co]
  bf16* const As = smem + 2 * S2_BN * S2_BK;  // [2][brows][64 co]
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int l16 = lane & 15;
  const int kgrp = lane >> 4;
  const int mb = blockIdx.x / ntn;
  const int nb = blockIdx.x - mb * ntn;
  const int q0 = mb * S2_BM, n0 = nb * S2_BN;

  const int srow = tid >> 3, sch = tid & 7;
  const int sto = s2_swz(srow, sch);
  // band row b is virtual pixel q0 + b: its dY pixel, -1 = zeros, -2 = beyond
  int pix[S2_MAXU];
#pragma unroll
  for (int u = 0; u < S2_MAXU; ++u) {
    const int b = srow + 32 * u;
    int n, i, j;
    pix[u] = -2;
    if (b < brows)
      pix[u] = c3s2_cell((long long)q0 + b, g, n, i, j)
                   ? (n * g.Ho + i) * g.Wo + j : -1;
  }
  const bf16* const pa = dY + sch * 8;
  const bf16* const pb = Wf + ((long long)n0 + srow) * 9 * Cout + sch * 8;
  const int bstep = 32 * 9 * Cout;
  const bf16x8 zv = {(bf16)0.0f, (bf16)0.0f, (bf16)0.0f, (bf16)0.0f,
                     (bf16)0.0f, (bf16)0.0f, (bf16)0.0f, (bf16)0.0f};
  const int bo0 = l16 * S2_BK + ((kgrp ^ (l16 & 7)) << 3);
  const int arow = wave * 32 + l16;

  f32x4 acc[2][4];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[m][c] = (f32x4)0.0f;

  bf16x8 ra[S2_MAXU], rb[2];
  int kh, kw;

#define S2_BAND_LOAD(cof)                                                   \
  {                                                                         \
    _Pragma("unroll") for (int u = 0; u < S2_MAXU; ++u)                     \
      ra[u] = pix[u] >= 0 ? *reinterpret_cast<const bf16x8*>(               \
                                pa + (long long)pix[u] * Cout + (cof))      \
                          : zv;                                             \
  }
  // K offset of tap k's 64 x 64 tile of Wf in chunk c
#define S2_WF_OFF(k, c)                                                     \
  (s2_tap(ph, pw, (k), kh, kw), (8 - (3 * kh + kw)) * Cout + (c) * S2_BK)

  if (phase_mask & 1) {
    S2_BAND_LOAD(0)
    s2_w_load(rb, pb, bstep, S2_WF_OFF(0, 0));
    s2_band_store(ra, pix, As, sto);
    s2_w_store(rb, Bs, sto);
  }
  __syncthreads();

  const int nch = Cout / S2_BK;
  int buf = 0;  // parity of the step
#pragma unroll 1
  for (int c = 0; c < nch; ++c) {
    const bool nextc = c + 1 < nch;
#pragma unroll 1
    for (int k = 0; k < ntaps; ++k) {
      const bool last = k + 1 == ntaps;
      const bool more = !last || nextc;
      if (more && (phase_mask & 1))
        s2_w_load(rb, pb, bstep,
                  last ? S2_WF_OFF(0, c + 1) : S2_WF_OFF(k + 1, c));
      // the next chunk's band: under this chunk's MFMAs
      if (k == 0 && nextc && (phase_mask & 1)) S2_BAND_LOAD((c + 1) * S2_BK)
      if (phase_mask & 4) {
        s2_tap(ph, pw, k, kh, kw);
        s2_mfma_step(acc, As + (c & 1) * brows * S2_BK,
                     Bs + buf * S2_BN * S2_BK,
                     arow + (kh ? 0 : g.Wp) + (kw ? 0 : 1), kgrp, bo0);
      }
      // the other band buffer was last read by chunk c - 1, behind a barrier
      if (last && nextc && (phase_mask & 1))
        s2_band_store(ra, pix, As + ((c + 1) & 1) * brows * S2_BK, sto);
      if (more && (phase_mask & 1))
        s2_w_store(rb, Bs + (buf ^ 1) * S2_BN * S2_BK, sto);
      __syncthreads();  // this step is read, the next is in place
      buf ^= 1;
    }
  }
#undef S2_BAND_LOAD
#undef S2_WF_OFF
  if (!(phase_mask & 2)) return;

  int n, i, j, opix = -1;
  if (c3s2_cell((long long)q0 + wave * 32 + (lane & 31), g, n, i, j) &&
      2 * i + ph < g.H && 2 * j + pw < g.W)
    opix = (n * g.H + 2 * i + ph) * g.W + 2 * j + pw;
  s2_epilogue<false>(acc, opix, smem, dX, Cin, n0, nullptr, 0, mb);
}

// M-blocks (= statistics slots per channel): ceil(N*(Ho+1)*(Wo+1) / 128)
extern "C" int conv3x3_s2_m_blocks(long long N, long long H, long long W) {
  return (int)((N * ((H + 1) / 2 + 1) * ((W + 1) / 2 + 1) + S2_BM - 1) /
               S2_BM);
}

// weight tiles + two bands, in bytes
static size_t conv3x3_s2_lds_bytes(int Wo) {
  return (size_t)(2 * S2_BN + 2 * (S2_BM + Wo + 2)) * S2_BK * sizeof(bf16);
}

// above 64 KB a kernel's dynamic LDS limit has to be raised before launch
template <typename K>
static void conv3x3_s2_allow_lds(K kernel, size_t lds) {
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds);
}

// x [N,H,W,Cin], w [Cout,3,3,Cin], out [N,Ho,Wo,Cout]. ``partial`` null: no
// statistics. Non-null: fp32 [2*Cout][conv3x3_s2_m_blocks(N, H, W)].
extern "C" void launch_conv3x3_s2_fwd(const void* x, const void* w, void* out,
                                      float* partial, int N, int H, int W,
                                      int Cin, int Cout, hipStream_t stream,
                                      int phase_mask) {
  const C3S2Geo g = c3s2_geo(N, H, W);
  const int ntn = Cout / S2_BN;
  const dim3 grid(conv3x3_s2_m_blocks(N, H, W) * ntn), block(256);
  const size_t lds = conv3x3_s2_lds_bytes(g.Wo);
  if (partial) {
    conv3x3_s2_allow_lds(conv3x3_s2_fwd_kernel<true>, lds);
    hipLaunchKernelGGL(conv3x3_s2_fwd_kernel<true>, grid, block, lds, stream,
                       (const bf16*)x, (const bf16*)w, (bf16*)out, partial,
                       Cin, Cout, ntn, phase_mask, g);
  } else {
    conv3x3_s2_allow_lds(conv3x3_s2_fwd_kernel<false>, lds);
    hipLaunchKernelGGL(conv3x3_s2_fwd_kernel<false>, grid, block, lds, stream,
                       (const bf16*)x, (const bf16*)w, (bf16*)out,
                       (float*)nullptr, Cin, Cout, ntn, phase_mask, g);
  }
}

// dx [N,H,W,Cin] from dy [N,Ho,Wo,Cout] and wf [Cin,3,3,Cout], the rotated
// repack launch_conv3x3_wflip writes
extern "C" void launch_conv3x3_s2_dgrad(const void* dy, const void* wf,
                                        void* dx, int N, int H, int W,
                                        int Cin, int Cout, hipStream_t stream,
                                        int phase_mask) {
  const C3S2Geo g = c3s2_geo(N, H, W);
  const int ntn = Cin / S2_BN;
  const dim3 grid(conv3x3_s2_m_blocks(N, H, W) * ntn, 4), block(256);
  const size_t lds = conv3x3_s2_lds_bytes(g.Wo);
  conv3x3_s2_allow_lds(conv3x3_s2_dgrad_kernel, lds);
  hipLaunchKernelGGL(conv3x3_s2_dgrad_kernel, grid, block, lds, stream,
                     (const bf16*)dy, (const bf16*)wf, (bf16*)dx, Cin, Cout,
                     ntn, phase_mask, g);
}
