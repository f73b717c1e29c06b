// Hand-written MFMA pointwise (1x1, stride 1 and 2) convolution for gfx950,
// NHWC bf16: forward, forward with BatchNorm statistics in the epilogue,
// data-grad, and (second half of this file) a split-K weight-grad. The
// stride-2 variants (the downsample projections; end of this comment) are
// the S2 = true instantiations of the same two kernel templates.
//
// Why: two thirds of a Bottleneck network's convs are 1x1 (the reference
// trains torchvision resnet50, deep_learning/
// 2.distributed-data-loading-petastorm.py:150), and in channels-last
// storage a stride-1 1x1 conv is a plain GEMM with both operands
// contiguous along the reduction axis:
//
//   fwd:    Y [M][Cout] = X [M][Cin]  . W[Cout][Cin]^T     (M = N*H*W)
//   dgrad:  dX[M][Cin]  = dY[M][Cout] . W[Cout][Cin]
//
// No im2col, no band, no halo. Every such conv is followed by a BN whose
// reduce pass reads the whole output back only to sum it; the stats
// variant sums the bf16 values it stores into one [2C][nblocks] slot per
// M-block (the layout bn_fwd_finalize reads), as the stem conv does.
//
// One templated body on v_mfma_f32_16x16x32_bf16 (A row = lane&15, B col
// = lane&15, k-slice = 8*(lane>>4)+j; D col = lane&15, row =
// 4*(lane>>4)+reg), fp32 accumulation:
//   * work split: 256 threads own a 128 x 64 output tile, a wave 32 rows
//     x 64 columns (2 x 4 accumulator tiles, 32 VGPRs). blockIdx.x walks
//     the column tiles of one M-block first, so the A rows of an M-block
//     come from HBM once and from L2 for the other column tiles, and the
//     weight (<= 8 MB) stays L2-resident.
//   * data movement: K-step 64. A (128 x 64) and B (64 x 64) tiles go
//     global -> registers -> LDS as 16-byte loads and stores, four plus
//     two per thread, double-buffered: the loads of step k+1 are issued
//     before the MFMAs of step k and stored after them, one barrier per
//     K-step. Rows at or beyond M are loaded as zeros.
//   * LDS rows are 128 bytes with the 16-byte chunk index XOR-ed with
//     (row & 7) instead of padded: eight consecutive rows put the same
//     logical chunk on eight different bank groups, and two buffers of
//     A + B are exactly 48 KB (a 72-element padded stride needs 54 KB and
//     loses the third block per CU).
//   * dgrad contracts over Cout, the STRIDED index of W as it lies in
//     memory. Its B tile is staged as it lies ([co][ci], 16-byte loads
//     along ci) and read with the transposing ds_read_b64_tr_b16: 16
//     lanes hand in four rows of 16 columns, each lane gets one column's
//     four K values; two reads make one operand in the A operand's own K
//     order (k = 8*(lane>>4) + 4*t + i). The XOR swizzle works on 16-byte
//     chunks and a transposed read takes 8 bytes inside one, so it holds
//     for both access patterns. EXEC is all ones at every transposed
//     read: the M tail is masked at the global loads and stores only.
//   * epilogue: accumulators are rounded to bf16 and transposed through a
//     wave-private LDS tile so the global stores are 16 bytes per lane
//     along the channel axis. Statistics: each lane sums value and
//     square of the ROUNDED outputs of its 8 rows per column, the four
//     lanes sharing a column add by shuffle, the four waves through LDS
//     in a fixed order; one thread per column writes the two slots. No
//     atomics: bit-reproducible. Zero rows add nothing to the sums.
//
// Stride 2 (X [N,H,W,Cin]; Y, dY [N,Ho,Wo,Cout], Ho = (H+1)/2, Wo =
// (W+1)/2, M' = N*Ho*Wo): the same GEMMs over M' rows with the rows of
// the large map gathered. Output pixel m' = (n, ho, wo) pairs with input
// pixel (n, 2ho, 2wo), still Cin contiguous values, so every load and
// store stays 16 bytes along the channel axis and the LDS tiles, the
// statistics epilogue and the partial layouts are the stride-1 ones.
//   * row map: m' -> (n*H + 2ho)*W + 2wo by two 32-bit divisions (by
//     Ho*Wo, then by Wo), each ONE v_mul_hi_u32 with a host-computed
//     floor(2^32 / d) passed in the kernel arguments plus one conditional
//     correction (the product underestimates the quotient by at most one
//     for every 32-bit dividend). No 64-bit division, no loop over image
//     rows: the cost is the same for every Wo.
//   * forward: the four A rows a thread stages keep four gathered base
//     pointers computed once before the K loop (8 VGPRs).
//   * data-grad: the A operand (dY) is contiguous; the epilogue scatters.
//     The 2x2 input cells (2ho..2ho+1, 2wo..2wo+1), clipped to H and W,
//     tile the large map exactly, so the lanes that hold 16 bytes of
//     product row m' store them to the cell's top-left pixel and 16-byte
//     zero vectors to the cell's other in-bounds pixels: every element of
//     dX is written exactly once by this one launch (no memset, no
//     atomics, dX may be uninitialised).
//   * weight-grad: the dY panel is contiguous, the X panel row of each
//     32-row K-step comes through the row map, once per thread per step.
// S2 is a template parameter and the stride-1 geometry argument an empty
// struct: the stride-1 instantiations compile to the code they had.
#include <hip/hip_runtime.h>
#include "conv_mfma.h"

#include <type_traits>

#define BM 128                  // output rows per block
#define BN 64                   // output columns per block
#define BK 64                   // K-step
#define OTROW 72                // epilogue tile row stride (els): 144 B

enum { C1_FWD = 0, C1_FWD_STATS = 1, C1_DGRAD = 2 };

// element offset of 16-byte chunk ``ch`` of row ``row`` in a [rows][BK] tile
__device__ __forceinline__ int swz(int row, int ch) {
  return row * BK + ((ch ^ (row & 7)) << 3);
}

// Stride-2 geometry: the large map's H and W, the small map's Wo and
// Ho*Wo, and floor(2^32 / d) for those two divisors (2^32 - 1 for d = 1).
struct C1S2 {
  int H, W, Wo, HoWo;
  unsigned rWo, rHoWo;
};
struct C1S1 {};  // stride 1 has no geometry
template <bool S2>
using C1Geo = typename std::conditional<S2, C1S2, C1S1>::type;

// q = m / d, m -= q * d, for any 32-bit m: m * floor(2^32/d) / 2^32 lies
// in (m/d - 1, m/d], so its floor is the quotient or one below it
__device__ __forceinline__ unsigned s2_divmod(unsigned& m, unsigned d,
                                              unsigned rd) {
  unsigned q = __umulhi(m, rd);
  m -= q * d;
  if (m >= d) {
    m -= d;
    ++q;
  }
  return q;
}

// small-map row m' = (n*Ho + ho)*Wo + wo -> (n, 2ho, 2wo) of the large map
__device__ __forceinline__ void s2_pixel(unsigned m, const C1S2& g,
                                         unsigned& n, unsigned& hi,
                                         unsigned& wi) {
  n = s2_divmod(m, (unsigned)g.HoWo, g.rHoWo);
  hi = 2 * s2_divmod(m, (unsigned)g.Wo, g.rWo);
  wi = 2 * m;
}

// ... -> its row in the large map (below 2^31: the bindings check)
__device__ __forceinline__ unsigned s2_row(unsigned m, const C1S2& g) {
  unsigned n, hi, wi;
  s2_pixel(m, g, n, hi, wi);
  return (n * g.H + hi) * g.W + wi;
}

// Out[M][N] = A[M][K] . B, with B = W[N][K] (C1_FWD*) or W[K][N]
// (C1_DGRAD). grid = ceil(M / BM) * (N / BN), column tiles fastest.
// phase_mask: 1 = global loads + LDS staging, 4 = MFMA, 2 = epilogue.
// S2: M counts the small map's rows; the forward gathers its A rows from
// the large map and the data-grad scatters its output rows into it.
template <int MODE, bool S2 = false>
__global__ __launch_bounds__(256, 3) void conv1x1_gemm_kernel(
    const bf16* __restrict__ A, const bf16* __restrict__ B,
    bf16* __restrict__ Out,
    float* __restrict__ partial,  // [2*N][ceil(M / BM)], C1_FWD_STATS only
    int M, int N, int K, int ntn, int phase_mask, const C1Geo<S2> g) {
  constexpr bool GATHER = S2 && MODE != C1_DGRAD;
  __shared__ __attribute__((aligned(16))) bf16 smem[2 * (BM + BN) * BK];
  bf16* const As = smem;                // [2][BM * BK]
  bf16* const Bs = smem + 2 * BM * BK;  // [2][BN * BK]
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int l16 = lane & 15;
  const int kgrp = lane >> 4;
  const int mb = blockIdx.x / ntn;
  const int nb = blockIdx.x - mb * ntn;
  const int m0 = mb * BM, n0 = nb * BN;
  const int nmb = gridDim.x / ntn;

  // staging: thread -> 16-byte chunk (tid & 7) of tile rows (tid >> 3) +
  // 32u; eight neighbours cover one 128-byte row. The swizzle term is the
  // same for every u (32u is a multiple of 8).
  const int srow = tid >> 3, sch = tid & 7;
  const int sto = swz(srow, sch);
  const bf16* pa = A + ((long long)m0 + srow) * K + sch * 8;
  const bf16* pb = MODE == C1_DGRAD
      ? B + (long long)srow * N + n0 + sch * 8
      : B + ((long long)n0 + srow) * K + sch * 8;
  const int bstep = MODE == C1_DGRAD ? 32 * N : 32 * K;  // 32 B-tile rows
  const int bkstep = MODE == C1_DGRAD ? BK * N : BK;     // one K-step
  const bf16x8 zv = {(bf16)0.0f, (bf16)0.0f, (bf16)0.0f, (bf16)0.0f,
                     (bf16)0.0f, (bf16)0.0f, (bf16)0.0f, (bf16)0.0f};
  bool alive[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) alive[u] = m0 + srow + 32 * u < M;
  // stride-2 forward: the four A rows lie at gathered rows of the large map
  const bf16* pag[4];
  if constexpr (GATHER) {
#pragma unroll
    for (int u = 0; u < 4; ++u)
      pag[u] = alive[u]
          ? A + (long long)s2_row(m0 + srow + 32 * u, g) * K + sch * 8
          : A;
  }

  // operand addressing (element offsets inside one tile)
  const int sw = l16 & 7;               // row & 7 of every row this lane reads
  const int fo0 = (kgrp ^ sw) << 3;     // chunk kgrp (K 0..31)
  const int fo1 = fo0 ^ 32;             // chunk 4 + kgrp (K 32..63)
  const int arow = (wave * 32 + l16) * BK;
  const int brow = l16 * BK;
  // dgrad: transposed read t takes rows 8*kgrp + 4t + q, columns 4p..4p+3
  // of column tile c: chunk 2c + (p >> 1), swizzled by (4t + q)
  const int q = l16 >> 2, p = l16 & 3;
  const int tro0 = (8 * kgrp + q) * BK + (p & 1) * 4;
  const int tro1 = tro0 + 4 * BK;
  const int trs0 = ((p >> 1) ^ q) << 3;
  const int trs1 = ((p >> 1) ^ (4 + q)) << 3;

  f32x4 acc[2][4];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[m][c] = (f32x4)0.0f;

  bf16x8 ra[4], rb[2];
  const int nks = K / BK;

#define C1_GLOAD(ks)                                                        \
  {                                                                         \
    _Pragma("unroll") for (int u = 0; u < 4; ++u) {                         \
      if constexpr (GATHER)                                                 \
        ra[u] = alive[u] ? *reinterpret_cast<const bf16x8*>(                \
                               pag[u] + (ks) * BK)                          \
                         : zv;                                              \
      else                                                                  \
        ra[u] = alive[u] ? *reinterpret_cast<const bf16x8*>(                \
                               pa + (long long)u * 32 * K + (ks) * BK)      \
                         : zv;                                              \
    }                                                                       \
    _Pragma("unroll") for (int u = 0; u < 2; ++u)                           \
      rb[u] = *reinterpret_cast<const bf16x8*>(                             \
          pb + (long long)u * bstep + (long long)(ks) * bkstep);            \
  }
#define C1_LSTORE(buf)                                                      \
  {                                                                         \
    _Pragma("unroll") for (int u = 0; u < 4; ++u)                           \
      *reinterpret_cast<bf16x8*>(As + (buf) * BM * BK + sto + u * 32 * BK) = \
          ra[u];                                                            \
    _Pragma("unroll") for (int u = 0; u < 2; ++u)                           \
      *reinterpret_cast<bf16x8*>(Bs + (buf) * BN * BK + sto + u * 32 * BK) = \
          rb[u];                                                            \
  }

  if (phase_mask & 1) {
    C1_GLOAD(0)
    C1_LSTORE(0)
  }
  __syncthreads();

#pragma unroll 1
  for (int ks = 0; ks < nks; ++ks) {
    const int buf = ks & 1;
    const bool more = ks + 1 < nks;
    if (more && (phase_mask & 1)) C1_GLOAD(ks + 1)
    if (phase_mask & 4) {
      const bf16* as = As + buf * BM * BK;
      const bf16* bs = Bs + buf * BN * BK;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int fo = kk ? fo1 : fo0;
        bf16x8 af[2], bfr[4];
#pragma unroll
        for (int m = 0; m < 2; ++m)
          af[m] = *reinterpret_cast<const bf16x8*>(
              as + arow + m * 16 * BK + fo);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          if (MODE == C1_DGRAD)
            bfr[c] = tr_frag(bs + kk * 32 * BK + tro0 + ((c * 16) ^ trs0),
                             bs + kk * 32 * BK + tro1 + ((c * 16) ^ trs1));
          else
            bfr[c] = *reinterpret_cast<const bf16x8*>(
                bs + brow + c * 16 * BK + fo);
        }
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int c = 0; c < 4; ++c)
            acc[m][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                af[m], bfr[c], acc[m][c], 0, 0, 0);
      }
    }
    if (more && (phase_mask & 1)) C1_LSTORE(buf ^ 1)
    __syncthreads();  // step ks is read, step ks+1 is in place
  }
#undef C1_GLOAD
#undef C1_LSTORE
  if (!(phase_mask & 2)) return;

  // D col = lane&15, row = 4*(lane>>4)+r: round, count into the
  // statistics, and transpose through the wave's own tile (the operand
  // buffers are free behind the loop's last barrier)
  bf16* tw = smem + wave * 32 * OTROW;
  float ssum[4] = {0.f, 0.f, 0.f, 0.f}, ssq[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const bf16 v = (bf16)acc[m][c][r];
        tw[(m * 16 + kgrp * 4 + r) * OTROW + c * 16 + l16] = v;
        if (MODE == C1_FWD_STATS) {
          const float f = (float)v;  // rows >= M are exact zeros
          ssum[c] += f;
          ssq[c] += f * f;
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
    const int row = m0 + wave * 32 + rl;
    const bf16x8 val = *reinterpret_cast<const bf16x8*>(tw + rl * OTROW + j8);
    if constexpr (S2 && MODE == C1_DGRAD) {
      // the row goes to the top-left pixel of its 2x2 cell of the large
      // map, zeros to the cell's other pixels inside H x W
      if (row < M) {
        unsigned n, hi, wi;
        s2_pixel(row, g, n, hi, wi);
        bf16* const o =
            Out + (long long)((n * g.H + hi) * g.W + wi) * N + n0 + j8;
        const bool right = (int)wi + 1 < g.W, below = (int)hi + 1 < g.H;
        const long long down = (long long)g.W * N;
        *reinterpret_cast<bf16x8*>(o) = val;
        if (right) *reinterpret_cast<bf16x8*>(o + N) = zv;
        if (below) *reinterpret_cast<bf16x8*>(o + down) = zv;
        if (right && below) *reinterpret_cast<bf16x8*>(o + down + N) = zv;
      }
    } else {
      if (row < M)
        *reinterpret_cast<bf16x8*>(Out + (long long)row * N + n0 + j8) = val;
    }
  }

  if (MODE == C1_FWD_STATS) {
    // the four row groups of a wave, then the four waves (fixed order),
    // then this M-block's slot of the block's 64 columns
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      ssum[c] += __shfl_xor(ssum[c], 16, 64);
      ssum[c] += __shfl_xor(ssum[c], 32, 64);
      ssq[c] += __shfl_xor(ssq[c], 16, 64);
      ssq[c] += __shfl_xor(ssq[c], 32, 64);
    }
    float* red = reinterpret_cast<float*>(smem + 4 * 32 * OTROW);
    if (kgrp == 0) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        red[wave * 2 * BN + c * 16 + l16] = ssum[c];
        red[wave * 2 * BN + BN + c * 16 + l16] = ssq[c];
      }
    }
    __syncthreads();
    if (tid < 2 * BN) {
      float t = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) t += red[w * 2 * BN + tid];
      const int ch = tid < BN ? n0 + tid : N + n0 + tid - BN;
      partial[(long long)ch * nmb + mb] = t;
    }
  }
}

// M-blocks (= statistics slots per channel) of the forward
extern "C" int conv1x1_m_blocks(long long M) {
  return (int)((M + BM - 1) / BM);
}

// ``partial`` null: no statistics. Non-null: fp32
// [2*Cout][conv1x1_m_blocks(M)], filled with the per-block channel sums.
extern "C" void launch_conv1x1_fwd(const void* x, const void* w, void* out,
                                   float* partial, long long M, int Cin,
                                   int Cout, hipStream_t stream,
                                   int phase_mask) {
  const int ntn = Cout / BN;
  const dim3 grid(conv1x1_m_blocks(M) * ntn), block(256);
  if (partial)
    hipLaunchKernelGGL(conv1x1_gemm_kernel<C1_FWD_STATS>, grid, block, 0,
                       stream, (const bf16*)x, (const bf16*)w, (bf16*)out,
                       partial, (int)M, Cout, Cin, ntn, phase_mask, C1S1{});
  else
    hipLaunchKernelGGL(conv1x1_gemm_kernel<C1_FWD>, grid, block, 0, stream,
                       (const bf16*)x, (const bf16*)w, (bf16*)out,
                       (float*)nullptr, (int)M, Cout, Cin, ntn, phase_mask,
                       C1S1{});
}

extern "C" void launch_conv1x1_dgrad(const void* dy, const void* w, void* dx,
                                     long long M, int Cin, int Cout,
                                     hipStream_t stream, int phase_mask) {
  const int ntn = Cin / BN;
  const dim3 grid(conv1x1_m_blocks(M) * ntn), block(256);
  hipLaunchKernelGGL(conv1x1_gemm_kernel<C1_DGRAD>, grid, block, 0, stream,
                     (const bf16*)dy, (const bf16*)w, (bf16*)dx,
                     (float*)nullptr, (int)M, Cin, Cout, ntn, phase_mask,
                     C1S1{});
}

// floor(2^32 / d), saturated for d = 1: the multiplier s2_divmod takes
static unsigned s2_recip(long long d) {
  const long long r = (1LL << 32) / d;
  return r > 0xffffffffLL ? 0xffffffffu : (unsigned)r;
}

static C1S2 s2_geom(int H, int W) {
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  return {H, W, Wo, Ho * Wo, s2_recip(Wo), s2_recip((long long)Ho * Wo)};
}

// rows of the small map: N * ((H+1)/2) * ((W+1)/2)
static long long conv1x1_s2_rows(long long N, long long H, long long W) {
  return N * ((H + 1) / 2) * ((W + 1) / 2);
}

// Stride 2: x [N,H,W,Cin] -> out [N,Ho,Wo,Cout]; ``partial`` as above with
// M' = conv1x1_s2_rows(N, H, W) in the place of M.
extern "C" void launch_conv1x1_s2_fwd(const void* x, const void* w, void* out,
                                      float* partial, int N, int H, int W,
                                      int Cin, int Cout, hipStream_t stream,
                                      int phase_mask) {
  const long long M = conv1x1_s2_rows(N, H, W);
  const int ntn = Cout / BN;
  const dim3 grid(conv1x1_m_blocks(M) * ntn), block(256);
  if (partial)
    hipLaunchKernelGGL((conv1x1_gemm_kernel<C1_FWD_STATS, true>), grid, block,
                       0, stream, (const bf16*)x, (const bf16*)w, (bf16*)out,
                       partial, (int)M, Cout, Cin, ntn, phase_mask,
                       s2_geom(H, W));
  else
    hipLaunchKernelGGL((conv1x1_gemm_kernel<C1_FWD, true>), grid, block, 0,
                       stream, (const bf16*)x, (const bf16*)w, (bf16*)out,
                       (float*)nullptr, (int)M, Cout, Cin, ntn, phase_mask,
                       s2_geom(H, W));
}

// Stride 2: dx [N,H,W,Cin] from dy [N,Ho,Wo,Cout]; writes all of dx.
extern "C" void launch_conv1x1_s2_dgrad(const void* dy, const void* w,
                                        void* dx, int N, int H, int W,
                                        int Cin, int Cout, hipStream_t stream,
                                        int phase_mask) {
  const long long M = conv1x1_s2_rows(N, H, W);
  const int ntn = Cin / BN;
  const dim3 grid(conv1x1_m_blocks(M) * ntn), block(256);
  hipLaunchKernelGGL((conv1x1_gemm_kernel<C1_DGRAD, true>), grid, block, 0,
                     stream, (const bf16*)dy, (const bf16*)w, (bf16*)dx,
                     (float*)nullptr, (int)M, Cin, Cout, ntn, phase_mask,
                     s2_geom(H, W));
}

// ---------------------------------------------------------------------
// Weight-grad:  dW[Cout][Cin] = sum_m dY[m][Cout] * X[m][Cin]   (m < M)
//
// The opposite of the GEMM above: the output is tiny (64x64 .. 2048x512),
// the reduction runs over M (up to 665k at batch 212), and M is the
// STRIDED index of both operands. So it has its own work split and its
// own operand path:
//   * work split: 256 threads own a TCO x TCI tile of dW and one chunk of
//     M (split-K). A side is 128 wide when its channel count is a multiple
//     of 128 and 64 otherwise (64, 192, 320, ...): four instantiations.
//     The four waves sit 2 x 2, a wave holds (TCI/32) x (TCO/32)
//     accumulator tiles (4 x 4 = 64 VGPRs at 128 x 128). blockIdx.x =
//     chunk * tiles + tile: the tiles of one chunk are neighbours in
//     launch order, so a chunk's rows come from HBM once and from L2 for
//     the other tiles.
//   * the MFMA computes dW^T: A = X^T (row = ci), B = dY (col = co). A
//     lane then holds four consecutive ci of one co, which is 16
//     contiguous bytes of part[chunk][co][ci]: the epilogue is plain
//     16-byte stores, no transpose through LDS. Every partial slot is
//     written by exactly one block; no atomics, bit-reproducible.
//   * K-step WK = 32 rows of m. Tiles are [WK][64-channel] panels staged
//     exactly as they lie in memory (16-byte loads along the channel axis,
//     rows at or beyond M load zeros), global -> registers -> LDS,
//     double-buffered, one barrier per step as in the GEMM body. WK = 32
//     and not 64: two buffers of a 128 + 128 tile are 32 KB (64 KB at 64,
//     which caps a CU at two blocks), and the staging registers are 16
//     instead of 32 next to 64 accumulators and 32 operand registers: the
//     128 x 128 instantiation compiles to 126 VGPRs, no scratch, which is
//     under the 128 that FOUR blocks per CU need (the issue budgeted 168
//     for three), so the launch bound pins four.
//   * both operands come out of LDS with ds_read_b64_tr_b16, the C1_DGRAD
//     B pattern: 16 lanes hand in four rows of 16 columns, two reads make
//     one operand with k = 8*(lane>>4) + 4t + i for A and B alike. EXEC is
//     all ones at every transposed read; the M tail is masked at the
//     global loads only.
//   * bank reasoning (not measured): a panel row is 128 bytes. One
//     transposed read touches rows 8g + 4t + q (g = lane>>4, q = 0..3), 32
//     bytes (one pair of 16-byte chunks) in each. With swz() the swizzle
//     term of those rows is 4t + q: q and q^1 only swap the two chunks of
//     one pair, and g does not enter, so the four rows of a 16-lane group
//     fall on two chunk pairs and the four groups on the same banks. wswz()
//     XORs the pair index with (row & 3) ^ (row>>3 & 1) and the chunk
//     inside the pair with (row>>2 & 1): the four rows of a group take the
//     four different pairs (a full 128 bytes, conflict-free if the LDS
//     serves 16 lanes per pass over 32 banks), and groups g, g^1 take
//     opposite pairs on rows of equal parity (conflict-free if it serves
//     32 lanes per pass over 64 banks, where odd rows sit in the upper
//     half). The 16-byte staging stores write whole rows, any chunk
//     permutation of which is conflict-free.
//
// conv1x1_wrw_reduce_kernel sums the chunk partials in fp32, rounds once
// to bf16 and stores, or adds into the bf16 values already there exactly
// as a bf16 tensor add of the rounded result would (accumulate mode: the
// kernel writes the flat grad view and AccumulateGrad has nothing to do).
// With few chunks one thread walks them in index order. With many (tiny
// dW, hundreds of chunks) that walk is one memory latency per batch on a
// handful of blocks, so `groups` threads share an element: each sums a
// contiguous run of chunks in index order, and the runs are added in
// index order through LDS. Fixed order either way.
#define WK 32                   // rows of m per K-step
#define WPANEL (WK * 64)        // elements of one [WK][64] panel
#define WRW_MIN_STEPS 4         // shortest chunk the default rule makes

// part[chunk][Cout][Cin] = sum over the chunk's rows. grid = chunks *
// tiles; spc = K-steps per chunk (the last chunk may be shorter, never
// empty). phase_mask: 1 = global loads + LDS staging, 4 = MFMA, 2 = epilogue.
// S2: M counts the rows of dY (the small map) and row m of the X panel is
// row s2_row(m) of the large map.
template <int TCO, int TCI, bool S2 = false>
__global__ __launch_bounds__(256, 4) void conv1x1_wrw_kernel(
    const bf16* __restrict__ X, const bf16* __restrict__ dY,
    float* __restrict__ part, int M, int Cin, int Cout, int ntci, int tiles,
    int spc, int phase_mask, const C1Geo<S2> g) {
  constexpr int PI = TCI / 64, PO = TCO / 64;  // panels per operand
  constexpr int IT = TCI / 32, OT = TCO / 32;  // accumulator tiles per wave
  constexpr int TILE = (PI + PO) * WPANEL;     // one buffer: X panels, dY panels
  __shared__ __attribute__((aligned(16))) bf16 smem[2 * TILE];
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int l16 = lane & 15;
  const int kgrp = lane >> 4;
  const int chunk = blockIdx.x / tiles;
  const int tile = blockIdx.x - chunk * tiles;
  const int to = tile / ntci;
  const int co0 = to * TCO, ci0 = (tile - to * ntci) * TCI;
  const int s0 = chunk * spc;
  const int ns = min(spc, (M + WK - 1) / WK - s0);

  // staging: thread -> 16-byte chunk (tid & 7) of panel row (tid >> 3);
  // 256 threads cover one panel, eight neighbours one 128-byte row
  const int srow = tid >> 3, sch = tid & 7;
  const int sto = wswz(srow, sch);
  const int mrow = s0 * WK + srow;
  const bf16* px = S2 ? X + ci0 + sch * 8  // the row is added per K-step
                      : X + (long long)mrow * Cin + ci0 + sch * 8;
  const bf16* py = dY + (long long)mrow * Cout + co0 + sch * 8;
  const bf16x8 zv = {(bf16)0.0f, (bf16)0.0f, (bf16)0.0f, (bf16)0.0f,
                     (bf16)0.0f, (bf16)0.0f, (bf16)0.0f, (bf16)0.0f};

  // transposed read t takes rows 8*kgrp + 4t + q, columns 4p..4p+3 of
  // column tile c: chunk 2c + (p >> 1), swizzled by wswz's term of that row
  const int q = l16 >> 2, p = l16 & 3;
  const int fq = (q ^ (kgrp & 1)) << 1;
  const int tro0 = (8 * kgrp + q) * 64 + (p & 1) * 4;
  const int tro1 = tro0 + 4 * 64;
  const int trs0 = ((p >> 1) ^ fq) << 3;
  const int trs1 = ((p >> 1) ^ (fq | 1)) << 3;
  // first channel of the wave's quarter inside the block tile
  const int wci = (wave & 1) * (TCI / 2), wco = (wave >> 1) * (TCO / 2);

  f32x4 acc[IT][OT];
#pragma unroll
  for (int i = 0; i < IT; ++i)
#pragma unroll
    for (int j = 0; j < OT; ++j) acc[i][j] = (f32x4)0.0f;

  bf16x8 rx[PI], ry[PO];

#define W_GLOAD(ks)                                                         \
  {                                                                         \
    const bool alive = mrow + (ks) * WK < M;                                \
    const bf16* pxk;                                                        \
    if constexpr (S2)                                                       \
      pxk = px + (long long)s2_row(mrow + (ks) * WK, g) * Cin;              \
    else                                                                    \
      pxk = px + (long long)(ks) * WK * Cin;                                \
    _Pragma("unroll") for (int u = 0; u < PI; ++u)                          \
      rx[u] = alive ? *reinterpret_cast<const bf16x8*>(pxk + u * 64) : zv;  \
    _Pragma("unroll") for (int u = 0; u < PO; ++u)                          \
      ry[u] = alive ? *reinterpret_cast<const bf16x8*>(                     \
                          py + (long long)(ks) * WK * Cout + u * 64)        \
                    : zv;                                                   \
  }
#define W_LSTORE(buf)                                                       \
  {                                                                         \
    _Pragma("unroll") for (int u = 0; u < PI; ++u)                          \
      *reinterpret_cast<bf16x8*>(smem + (buf) * TILE + u * WPANEL + sto) =  \
          rx[u];                                                            \
    _Pragma("unroll") for (int u = 0; u < PO; ++u)                          \
      *reinterpret_cast<bf16x8*>(smem + (buf) * TILE + (PI + u) * WPANEL +  \
                                 sto) = ry[u];                              \
  }

  if (phase_mask & 1) {
    W_GLOAD(0)
    W_LSTORE(0)
  }
  __syncthreads();

#pragma unroll 1
  for (int ks = 0; ks < ns; ++ks) {
    const int buf = ks & 1;
    const bool more = ks + 1 < ns;
    if (more && (phase_mask & 1)) W_GLOAD(ks + 1)
    if (phase_mask & 4) {
      const bf16* xs = smem + buf * TILE;
      const bf16* ys = xs + PI * WPANEL;
      bf16x8 xf[IT], yf[OT];
#pragma unroll
      for (int i = 0; i < IT; ++i) {
        const int col = wci + i * 16;  // panel col >> 6, column tile (col >> 4) & 3
        const bf16* pn = xs + (col >> 6) * WPANEL;
        xf[i] = tr_frag(pn + tro0 + ((col & 48) ^ trs0),
                        pn + tro1 + ((col & 48) ^ trs1));
      }
#pragma unroll
      for (int j = 0; j < OT; ++j) {
        const int col = wco + j * 16;
        const bf16* pn = ys + (col >> 6) * WPANEL;
        yf[j] = tr_frag(pn + tro0 + ((col & 48) ^ trs0),
                        pn + tro1 + ((col & 48) ^ trs1));
      }
#pragma unroll
      for (int i = 0; i < IT; ++i)
#pragma unroll
        for (int j = 0; j < OT; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              xf[i], yf[j], acc[i][j], 0, 0, 0);
    }
    if (more && (phase_mask & 1)) W_LSTORE(buf ^ 1)
    __syncthreads();  // step ks is read, step ks+1 is in place
  }
#undef W_GLOAD
#undef W_LSTORE
  if (!(phase_mask & 2)) return;

  // D row = 4*(lane>>4) + r is ci, D col = lane&15 is co: the four
  // registers of a tile are 16 contiguous bytes of part[chunk][co][...]
  float* const my = part + ((long long)chunk * Cout + co0 + wco + l16) * Cin +
                    ci0 + wci + 4 * kgrp;
#pragma unroll
  for (int i = 0; i < IT; ++i)
#pragma unroll
    for (int j = 0; j < OT; ++j)
      *reinterpret_cast<f32x4*>(my + (long long)j * 16 * Cin + i * 16) =
          acc[i][j];
}

// dw[e] = bf16(sum_c part[c][e]), or in accumulate mode
// bf16(float(dw[e]) + float(bf16(sum))). 256 threads = groups x (256 /
// groups) 16-byte columns; grid = nel / (4 * (256 / groups)); nel is a
// multiple of 4096 and groups a power of two <= 16, so nothing is ragged.
__global__ __launch_bounds__(256) void conv1x1_wrw_reduce_kernel(
    const float* __restrict__ part, bf16* __restrict__ dw, long long nel,
    int chunks, int groups, int accumulate) {
  __shared__ f32x4 red[256];
  const int tid = threadIdx.x;
  const int cols = 256 / groups;
  const int g = tid / cols, col = tid - g * cols;
  const long long e0 = ((long long)blockIdx.x * cols + col) * 4;
  const int per = (chunks + groups - 1) / groups;
  int c = g * per;
  const int c1 = min(chunks, c + per);
  const float* p = part + e0;
  f32x4 s = (f32x4)0.0f;
  // eight 16-byte loads in flight, added in chunk order
  for (; c + 8 <= c1; c += 8) {
    f32x4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u)
      v[u] = *reinterpret_cast<const f32x4*>(p + (long long)(c + u) * nel);
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; c < c1; ++c)
    s += *reinterpret_cast<const f32x4*>(p + (long long)c * nel);
  if (groups > 1) {
    red[tid] = s;
    __syncthreads();
    if (g != 0) return;
    for (int k = 1; k < groups; ++k) s += red[k * cols + col];
  }
  typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
  bf16x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = (bf16)s[e];
  if (accumulate) {
    const bf16x4 old = *reinterpret_cast<const bf16x4*>(dw + e0);
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (bf16)((float)old[e] + (float)o[e]);
  }
  *reinterpret_cast<bf16x4*>(dw + e0) = o;
}

// The reduce over ``nel`` elements (a multiple of 4096) of ``nchunks``
// partials; conv3x3wrw.hip launches it for its [Cout][9][Cin] partials too.
extern "C" void launch_conv_wrw_reduce(const float* part, void* dw,
                                       long long nel, int nchunks,
                                       int accumulate, hipStream_t stream) {
  int groups = 1;  // about 16 chunks per thread, at most 16 groups
  while (groups < 16 && nchunks > 16 * groups) groups *= 2;
  hipLaunchKernelGGL(conv1x1_wrw_reduce_kernel,
                     dim3((unsigned)(nel / (4 * (256 / groups)))), dim3(256),
                     0, stream, part, (bf16*)dw, nel, nchunks, groups,
                     accumulate);
}

static int wrw_side(int c) { return c % 128 == 0 ? 128 : 64; }

static int wrw_tiles(int Cin, int Cout) {
  return (Cin / wrw_side(Cin)) * (Cout / wrw_side(Cout));
}

// Chunk count for a request. req > 0 forces it (clamped to the K-steps);
// req == 0 takes the smallest count that puts about two blocks on every
// CU of the current device, with chunks of at least WRW_MIN_STEPS
// K-steps. Chunks are whole K-steps long and the value returned is the
// effective count ceil(steps / steps_per_chunk): no chunk is empty.
extern "C" int conv1x1_wrw_chunks(long long M, int Cin, int Cout, int req) {
  const long long steps = (M + WK - 1) / WK;
  long long n = req;
  if (req <= 0) {
    int dev = 0, cus = 0;  // of the current device: callers set it
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                              dev) != hipSuccess || cus <= 0)
      return -1;
    const int tiles = wrw_tiles(Cin, Cout);
    n = (2 * cus + tiles - 1) / tiles;
    if (n > steps / WRW_MIN_STEPS) n = steps / WRW_MIN_STEPS;
  }
  if (n > steps) n = steps;
  if (n < 1) n = 1;
  const long long spc = (steps + n - 1) / n;
  return (int)((steps + spc - 1) / spc);
}

// ``nchunks`` is a value conv1x1_wrw_chunks returned; part holds
// nchunks * Cout * Cin floats, every one of which is written.
template <bool S2>
static void wrw_launch(const void* x, const void* dy, float* part, void* dw,
                       long long M, int Cin, int Cout, int nchunks,
                       int accumulate, hipStream_t stream, int phase_mask,
                       const C1Geo<S2> g) {
  const int tci = wrw_side(Cin), tco = wrw_side(Cout);
  const int ntci = Cin / tci, tiles = wrw_tiles(Cin, Cout);
  const long long steps = (M + WK - 1) / WK;
  const int spc = (int)((steps + nchunks - 1) / nchunks);
  const dim3 grid(nchunks * tiles), block(256);
#define W_LAUNCH(TCO, TCI)                                                  \
  hipLaunchKernelGGL((conv1x1_wrw_kernel<TCO, TCI, S2>), grid, block, 0,    \
                     stream, (const bf16*)x, (const bf16*)dy, part, (int)M, \
                     Cin, Cout, ntci, tiles, spc, phase_mask, g)
  if (tco == 128 && tci == 128) W_LAUNCH(128, 128);
  else if (tco == 128) W_LAUNCH(128, 64);
  else if (tci == 128) W_LAUNCH(64, 128);
  else W_LAUNCH(64, 64);
#undef W_LAUNCH
  launch_conv_wrw_reduce(part, dw, (long long)Cout * Cin, nchunks, accumulate,
                         stream);
}

extern "C" void launch_conv1x1_wrw(const void* x, const void* dy, float* part,
                                   void* dw, long long M, int Cin, int Cout,
                                   int nchunks, int accumulate,
                                   hipStream_t stream, int phase_mask) {
  wrw_launch<false>(x, dy, part, dw, M, Cin, Cout, nchunks, accumulate,
                    stream, phase_mask, C1S1{});
}

// Stride 2: x [N,H,W,Cin], dy [N,Ho,Wo,Cout]; ``nchunks`` is what
// conv1x1_wrw_chunks returned for M' = conv1x1_s2_rows(N, H, W).
extern "C" void launch_conv1x1_s2_wrw(const void* x, const void* dy,
                                      float* part, void* dw, int N, int H,
                                      int W, int Cin, int Cout, int nchunks,
                                      int accumulate, hipStream_t stream,
                                      int phase_mask) {
  wrw_launch<true>(x, dy, part, dw, conv1x1_s2_rows(N, H, W), Cin, Cout,
                   nchunks, accumulate, stream, phase_mask, s2_geom(H, W));
}
