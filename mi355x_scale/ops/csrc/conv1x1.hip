// Hand-written MFMA pointwise (1x1, stride 1) convolution for gfx950,
// NHWC bf16: forward, forward with BatchNorm statistics in the epilogue,
// and data-grad. Weight-grad stays on MIOpen.
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
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#define BM 128                  // output rows per block
#define BN 64                   // output columns per block
#define BK 64                   // K-step
#define OTROW 72                // epilogue tile row stride (els): 144 B

typedef __bf16 bf16;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;

enum { C1_FWD = 0, C1_FWD_STATS = 1, C1_DGRAD = 2 };

// element offset of 16-byte chunk ``ch`` of row ``row`` in a [rows][BK] tile
__device__ __forceinline__ int swz(int row, int ch) {
  return row * BK + ((ch ^ (row & 7)) << 3);
}

// one MFMA operand (8 K values per lane) from two transposed block reads
__device__ __forceinline__ bf16x8 tr_frag(const bf16* p0, const bf16* p1) {
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p0);
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p1);
  const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, v);
}

// Out[M][N] = A[M][K] . B, with B = W[N][K] (C1_FWD*) or W[K][N]
// (C1_DGRAD). grid = ceil(M / BM) * (N / BN), column tiles fastest.
// phase_mask: 1 = global loads + LDS staging, 4 = MFMA, 2 = epilogue.
template <int MODE>
__global__ __launch_bounds__(256, 3) void conv1x1_gemm_kernel(
    const bf16* __restrict__ A, const bf16* __restrict__ B,
    bf16* __restrict__ Out,
    float* __restrict__ partial,  // [2*N][ceil(M / BM)], C1_FWD_STATS only
    int M, int N, int K, int ntn, int phase_mask) {
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
    _Pragma("unroll") for (int u = 0; u < 4; ++u)                           \
      ra[u] = alive[u] ? *reinterpret_cast<const bf16x8*>(                  \
                             pa + (long long)u * 32 * K + (ks) * BK)        \
                       : zv;                                                \
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
    if (row < M)
      *reinterpret_cast<bf16x8*>(Out + (long long)row * N + n0 + j8) = val;
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
                       partial, (int)M, Cout, Cin, ntn, phase_mask);
  else
    hipLaunchKernelGGL(conv1x1_gemm_kernel<C1_FWD>, grid, block, 0, stream,
                       (const bf16*)x, (const bf16*)w, (bf16*)out,
                       (float*)nullptr, (int)M, Cout, Cin, ntn, phase_mask);
}

extern "C" void launch_conv1x1_dgrad(const void* dy, const void* w, void* dx,
                                     long long M, int Cin, int Cout,
                                     hipStream_t stream, int phase_mask) {
  const int ntn = Cin / BN;
  const dim3 grid(conv1x1_m_blocks(M) * ntn), block(256);
  hipLaunchKernelGGL(conv1x1_gemm_kernel<C1_DGRAD>, grid, block, 0, stream,
                     (const bf16*)dy, (const bf16*)w, (bf16*)dx,
                     (float*)nullptr, (int)M, Cin, Cout, ntn, phase_mask);
}
