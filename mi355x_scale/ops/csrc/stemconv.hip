// Hand-written MFMA stem convolution for gfx950: 7x7 stride-2 pad-3,
// Cin=3, Cout=64, NHWC bf16 (fwd + weight-grad; the stem input never
// needs a data-grad).
//
// Why: the ResNet stem is the one conv MIOpen leaves on a generic igemm
// tile (C=3 starves the GEMM K: K = 7*7*3 = 147) — measured 298 us fwd
// + ~294 us wrw per step at bs 212, ~7% of the whole flagship step
// (profiles/r01_bench_resnet18_fused_kernstats.md). A shape-special
// kernel treats it as the GEMM it is:
//
//   fwd:  out[px][co]  = sum_k  patch[px][k]   * w[co][k]     (M=N*HO*WO, N=64, K=147)
//   wrw:  dw[co][k]    = sum_px dy[px][co]     * patch[px][k] (M=64, N=147, K=N*HO*WO)
//
// on v_mfma_f32_16x16x32_bf16 (frag maps per cdna_hip_programming.md §3:
// A row = lane&15, B col = lane&15, k-slice = 8*(lane>>4)+j; C/D
// col = lane&15, row = 4*(lane>>4)+reg).
//
// Memory discipline (ablated, v1/v2 lessons):
//   v1: per-element GLOBAL im2col gather — one load+wait per element,
//       waves >80% stalled (SQ_WAIT_ANY), 2.4 ms.
//   v2: contiguous band stage + LDS->LDS im2col expansion — the MFMA
//       phase alone measured 108 us, but stage (637 us) and expand
//       (541 us) still dominated: serialized load->ds_write round trips.
//   v3 (this): each block owns ONE output row (n, ho); the 7-row input
//       band is staged with short4 vector copies into a PIXEL-PADDED
//       layout (edge zeros materialized, plus an all-zero 8th row that
//       absorbs the K-padding taps), so there is no expansion phase and
//       no bounds checks: the MFMA loop gathers its A-fragments straight
//       from the band at koff(k) + px*6.
//   wrw, r6: the element gather (56 two-byte LDS reads per 10 MFMAs) made
//       LDS instruction issue the bound, at 1.57 TB/s and a fraction of
//       the MFMA rate. stem_conv_wrw_kernel now reads both operands with
//       ds_read_b64_tr_b16 (16 eight-byte reads per 12 MFMAs) from a band
//       kept as two images 4 bytes out of phase, in a tap order of its
//       own; 257 -> 133 us per step (profiles/r06_stem_wrw_tr_kernstats.md).
//       The gather kernel stays as stem_conv_wrw_gather_kernel.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#define KH 7
#define KW 7
#define CI 3
#define CO 64
#define KTAP (KH * KW * CI)     // 147
#define KPAD 160                // 5 x K32 MFMA steps
#define KLDS 168                // padded weight-tile row stride
#define PXPAD 128               // padded output-row length (WO <= 128)
// band row: 4 zero pixels of lead (data starts 8B-aligned at el 12),
// 2*PXPAD+KW pixel taps, zero tail; rounded to short4 granularity
#define XTROW ((4 + 2 * PXPAD + KW + 4) * CI + 3)  // 816 els
#define XTOFF 12                // data starts at pixel 4 -> element 12
#define STRIDE 2
#define PADDING 3

typedef __bf16 bf16;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;

// Stage the 7-row band. ``prime``: zero the whole 8-row tile first (the
// data region is fully overwritten every call with the same W, so
// non-prime calls only re-zero row slots whose ih fell outside the
// image — the lead/tail pads and row 7 stay zero from the prime).
// Copies are flattened over (row, chunk) and register-batched 5 deep so
// the global loads pipeline instead of paying one latency each (the v2
// lesson). Callers barrier before the MFMA phase.
__device__ __forceinline__ void stage_band(
    const bf16* __restrict__ x, bf16* xt, int n, int ho, int H, int W,
    int tid, int nthreads, bool prime) {
  const int rowlen = W * CI;
  if (prime) {
    for (int i = tid; i < 8 * XTROW; i += nthreads) xt[i] = (bf16)0.0f;
  } else {
    for (int r = 0; r < KH; ++r) {
      const int ih = ho * STRIDE - PADDING + r;
      if (ih < 0 || ih >= H)
        for (int i = tid; i < rowlen; i += nthreads)
          xt[r * XTROW + XTOFF + i] = (bf16)0.0f;
    }
  }
  __syncthreads();
  if ((rowlen & 3) == 0) {
    const int nch = rowlen >> 2;
    const int total = KH * nch;
    const bf16x4 z = {(bf16)0.0f, (bf16)0.0f, (bf16)0.0f, (bf16)0.0f};
    for (int base = 0; base < total; base += nthreads * 5) {
      bf16x4 v[5];
      int rr[5], cc[5];
#pragma unroll
      for (int u = 0; u < 5; ++u) {
        const int i = base + tid + u * nthreads;
        v[u] = z;
        rr[u] = -1;
        if (i < total) {
          const int r = i / nch, c = i - r * nch;
          const int ih = ho * STRIDE - PADDING + r;
          rr[u] = r; cc[u] = c;
          if (ih >= 0 && ih < H)
            v[u] = reinterpret_cast<const bf16x4*>(
                x + ((long long)n * H + ih) * rowlen)[c];
        }
      }
#pragma unroll
      for (int u = 0; u < 5; ++u)
        if (rr[u] >= 0)
          reinterpret_cast<bf16x4*>(
              xt + rr[u] * XTROW + XTOFF)[cc[u]] = v[u];
    }
  } else {  // odd row length (test shapes): scalar fallback
    for (int r = 0; r < KH; ++r) {
      const int ih = ho * STRIDE - PADDING + r;
      if (ih < 0 || ih >= H) continue;
      const bf16* src = x + ((long long)n * H + ih) * rowlen;
      bf16* dst = xt + r * XTROW + XTOFF;
      for (int i = tid; i < rowlen; i += nthreads) dst[i] = src[i];
    }
  }
}

// Ring-band staging for the wrw row loop: consecutive output rows (same
// n) share 5 of their 7 input rows, so after a prime only the TWO new
// rows are staged per step. Row slot = ih & 7 (bitwise works for the
// negative top-edge ihs); invalid rows are zeroed in their slot. The
// K-padding taps (kh = 7) would alias a live slot, so the wrw fragment
// builder zero-selects k >= KTAP instead of reading a dedicated row.
__device__ __forceinline__ void stage_band_ring(
    const bf16* __restrict__ x, bf16* xt, int n, int ho, int H, int W,
    int tid, int nthreads, bool prime) {
  const int rowlen = W * CI;
  const int ih0 = ho * STRIDE - PADDING;
  const int rfirst = prime ? 0 : KH - STRIDE;  // prime: all 7; else last 2
  if ((rowlen & 3) == 0) {
    const int nch = rowlen >> 2;
    const int nrows = KH - rfirst;
    const int total = nrows * nch;
    const bf16x4 z = {(bf16)0.0f, (bf16)0.0f, (bf16)0.0f, (bf16)0.0f};
    for (int base = 0; base < total; base += nthreads * 5) {
      bf16x4 v[5];
      int ss[5], cc[5];
#pragma unroll
      for (int u = 0; u < 5; ++u) {
        const int i = base + tid + u * nthreads;
        v[u] = z;
        ss[u] = -1;
        if (i < total) {
          const int r = rfirst + i / nch, c = i - (i / nch) * nch;
          const int ih = ih0 + r;
          ss[u] = (ih & 7); cc[u] = c;
          if (ih >= 0 && ih < H)
            v[u] = reinterpret_cast<const bf16x4*>(
                x + ((long long)n * H + ih) * rowlen)[c];
        }
      }
#pragma unroll
      for (int u = 0; u < 5; ++u)
        if (ss[u] >= 0)
          reinterpret_cast<bf16x4*>(
              xt + ss[u] * XTROW + XTOFF)[cc[u]] = v[u];
    }
  } else {
    for (int r = rfirst; r < KH; ++r) {
      const int ih = ih0 + r;
      bf16* dst = xt + (ih & 7) * XTROW + XTOFF;
      if (ih >= 0 && ih < H) {
        const bf16* src = x + ((long long)n * H + ih) * rowlen;
        for (int i = tid; i < rowlen; i += nthreads) dst[i] = src[i];
      } else {
        for (int i = tid; i < rowlen; i += nthreads) dst[i] = (bf16)0.0f;
      }
    }
  }
}

// koff(k): element offset of tap k for pixel 0 in the padded band.
// tap iw = px*STRIDE - PADDING + kw -> element
// XTOFF + (px*STRIDE - PADDING + kw)*CI + ci
//   = (XTOFF - PADDING*CI) + px*(STRIDE*CI) + (kw*CI + ci)
// pad taps (k >= 147) resolve to kh = 7, the all-zero row.
__device__ __forceinline__ int koff_of(int k) {
  const int kh = k / (KW * CI);
  const int r21 = k - kh * (KW * CI);
  return kh * XTROW + (XTOFF - PADDING * CI) + r21;
}

// Pad the weights once per forward: [CO][KTAP] -> [CO][KPAD] (zeros in
// the MFMA K-padding taps). 20 KB — L1-resident for every fwd block, so
// the per-block LDS weight-tile refill (40 serialized loads/lane x
// 23744 blocks) disappears entirely.
extern "C" __global__ __launch_bounds__(256) void stem_pad_weights_kernel(
    const bf16* __restrict__ w, bf16* __restrict__ wp) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < CO * KPAD) {
    const int co = i / KPAD, k = i - co * KPAD;
    wp[i] = (k < KTAP) ? w[co * KTAP + k] : (bf16)0.0f;
  }
}

// ---------------------------------------------------------------- forward
// block = 256 threads (4 waves) = one output row; wave w computes px
// subtiles {2w, 2w+1}. LDS = band only (13 KB) -> many blocks/CU; the
// B-fragments read the padded weight buffer straight from global (the
// whole 20 KB tile lives in L1).
extern "C" __global__ __launch_bounds__(256) void stem_conv_fwd_kernel(
    const bf16* __restrict__ x,   // [N][H][W][CI]
    const bf16* __restrict__ wp,  // [CO][KPAD] padded (stem_pad_weights)
    bf16* __restrict__ out,       // [N][HO][WO][CO]
    int Nb, int H, int W, int HO, int WO, int phase_mask) {
  __shared__ bf16 xt[8 * XTROW];
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int n = blockIdx.x / HO;
  const int ho = blockIdx.x - n * HO;

  if (phase_mask & 1) {
    stage_band(x, xt, n, ho, H, W, tid, 256, true);
  }
  __syncthreads();
  if (!(phase_mask & 4)) return;

  f32x4 acc[2][4];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[m][c] = (f32x4)0.0f;

  const int row16 = lane & 15;
  const int kgrp = lane >> 4;
  const int pxb0 = (wave * 32 + row16) * (STRIDE * CI);
  const int pxb1 = (wave * 32 + 16 + row16) * (STRIDE * CI);
#pragma unroll
  for (int kk = 0; kk < KPAD / 32; ++kk) {
    bf16x8 bfrag[4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
      bfrag[c] = *reinterpret_cast<const bf16x8*>(
          wp + (c * 16 + row16) * KPAD + kk * 32 + kgrp * 8);
    bf16x8 f0, f1;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int ko = koff_of(kk * 32 + kgrp * 8 + j);
      f0[j] = xt[ko + pxb0];
      f1[j] = xt[ko + pxb1];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      acc[0][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          f0, bfrag[c], acc[0][c], 0, 0, 0);
      acc[1][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          f1, bfrag[c], acc[1][c], 0, 0, 0);
    }
  }

  // store: D col = lane&15 (co), row = 4*(lane>>4)+r (px within row)
  const long long rowbase = ((long long)n * HO + ho) * WO;
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int pxr = wave * 32 + m * 16 + kgrp * 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int px = pxr + r;
      if (px >= WO) continue;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        out[(rowbase + px) * CO + c * 16 + row16] = (bf16)acc[m][c][r];
    }
  }
}

// ------------------------------------------- forward + BN batch statistics
// v4: a block owns FWD_ROWS consecutive output rows of ONE image (tail
// chunk shorter when FWD_ROWS does not divide HO). What changes against
// the kernel above, with the MFMA sequence itself untouched (same
// operands, same K order -> bit-identical bf16 output):
//   * the whole (2*rows+5)-row input band is staged ONCE, pads and
//     out-of-image rows written as zeros in the same pass (no separate
//     zeroing pass, no barrier between them, one barrier per block);
//     neighbouring output rows share five of seven input rows, so the
//     input is read ~1.3x instead of 3.5x and the row loop is barrier-free;
//   * the 20 weight B-fragments live in registers across the row loop
//     (80 VGPRs) instead of being re-read from L1 for every row: 80 KB of
//     vector-memory traffic per output row against 14 KB of output;
//   * the D fragments go through a wave-private LDS tile and leave as
//     16-byte-per-lane stores on consecutive addresses (1 KB per
//     wavefront instruction; the old epilogue issued 32 two-byte stores
//     per lane, four 32-byte runs per instruction);
//   * while the rounded values are in registers, each lane accumulates
//     sum / sum-of-squares for its four channels (fp32, px >= WO
//     excluded); after the row loop: lanes -> waves -> ONE slot of the
//     channel-major [2*CO][nblocks] partial layout bn_fwd_finalize_kernel
//     reads. No atomics, no cross-block traffic: fixed summation order,
//     deterministic under graph replay.
// LDS: band 21 rows (34,272 B) + 4 wave tiles (18,432 B) = 52,704 B ->
// 3 blocks/CU, which is also what the register budget (168) allows.
#define FWD_ROWS 8
#define FWD_BAND_ROWS (2 * FWD_ROWS + KH - STRIDE)   // 21
#define OTROW 72   // tile row stride (els): 144 B keeps the four px
                   // groups of a D-fragment store on disjoint banks and
                   // every 8-channel vector 16-byte aligned
#define XTCH (XTROW / 4)  // short4 chunks per band row (204)
// loads a thread keeps in flight while staging: 21 rows x 204 chunks over
// 256 threads is 17 per thread, so the whole band is one round trip
#define STAGE_DEPTH 17

// Stage ``nrows_in`` input rows starting at ih0 into the band, every
// element of every row written exactly once: data where the tap is
// inside the image, zero for the lead/tail pads and out-of-image rows.
__device__ __forceinline__ void stage_band_rows(
    const bf16* __restrict__ x, bf16* xt, int n, int ih0, int nrows_in,
    int H, int W, int tid, int nthreads) {
  const int rowlen = W * CI;
  if ((rowlen & 3) == 0) {
    const int nch = rowlen >> 2;
    const int total = nrows_in * XTCH;
    const bf16x4 z = {(bf16)0.0f, (bf16)0.0f, (bf16)0.0f, (bf16)0.0f};
    for (int base = 0; base < total; base += nthreads * STAGE_DEPTH) {
      bf16x4 v[STAGE_DEPTH];
#pragma unroll
      for (int u = 0; u < STAGE_DEPTH; ++u) {
        const int i = base + tid + u * nthreads;
        v[u] = z;
        if (i < total) {
          const int r = i / XTCH, c = i - r * XTCH - XTOFF / 4;
          const int ih = ih0 + r;
          if (ih >= 0 && ih < H && c >= 0 && c < nch)
            v[u] = reinterpret_cast<const bf16x4*>(
                x + ((long long)n * H + ih) * rowlen)[c];
        }
      }
#pragma unroll
      for (int u = 0; u < STAGE_DEPTH; ++u) {
        const int i = base + tid + u * nthreads;
        if (i < total) reinterpret_cast<bf16x4*>(xt)[i] = v[u];
      }
    }
  } else {  // odd row length (test shapes): scalar fallback
    const int total = nrows_in * XTROW;
    for (int i = tid; i < total; i += nthreads) {
      const int r = i / XTROW, e = i - r * XTROW - XTOFF;
      const int ih = ih0 + r;
      bf16 v = (bf16)0.0f;
      if (ih >= 0 && ih < H && e >= 0 && e < rowlen)
        v = x[((long long)n * H + ih) * rowlen + e];
      xt[i] = v;
    }
  }
}

// grid = Nb * ceil(HO / FWD_ROWS); partial is fp32 [2*CO][gridDim.x]
extern "C" __global__ __launch_bounds__(256, 3) void stem_conv_fwd_stats_kernel(
    const bf16* __restrict__ x,   // [N][H][W][CI]
    const bf16* __restrict__ wp,  // [CO][KPAD] padded (stem_pad_weights)
    bf16* __restrict__ out,       // [N][HO][WO][CO]
    float* __restrict__ partial,  // [2*CO][nblocks]
    int Nb, int H, int W, int HO, int WO, int nchunks, int phase_mask) {
  __shared__ __attribute__((aligned(16))) bf16 xt[FWD_BAND_ROWS * XTROW];
  __shared__ __attribute__((aligned(16))) bf16 ot[4 * 32 * OTROW];
  // byte offsets (relative to band row 2*rr, pixel 0) of the 40 taps a
  // lane gathers, one 40-entry run per k-group. Per-lane address math
  // hoisted out of the row loop costs 80 registers and spills the
  // weights; the table costs five broadcast 16-byte LDS reads per M-tile.
  __shared__ __attribute__((aligned(16))) unsigned short ktab[4 * KPAD / 4];
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int row16 = lane & 15;
  const int kgrp = lane >> 4;
  const int n = blockIdx.x / nchunks;
  const int ho0 = (blockIdx.x - n * nchunks) * FWD_ROWS;
  const int rows = min(FWD_ROWS, HO - ho0);

  // weight fragments: issued first so their latency hides under staging
  bf16x8 bfrag[KPAD / 32][4];
#pragma unroll
  for (int kk = 0; kk < KPAD / 32; ++kk)
#pragma unroll
    for (int c = 0; c < 4; ++c)
      bfrag[kk][c] = *reinterpret_cast<const bf16x8*>(
          wp + (c * 16 + row16) * KPAD + kk * 32 + kgrp * 8);

  if (tid < 4 * KPAD / 4) {
    const int g = tid / (KPAD / 4), i = tid - g * (KPAD / 4);
    const int k = (i >> 3) * 32 + g * 8 + (i & 7);
    ktab[tid] = (unsigned short)(2 * koff_of(min(k, KTAP - 1)));
  }
  if (phase_mask & 1)
    stage_band_rows(x, xt, n, ho0 * STRIDE - PADDING,
                    rows * STRIDE + KH - STRIDE, H, W, tid, 256);
  __syncthreads();
  if (!(phase_mask & 4)) return;

  float ssum[4] = {0.f, 0.f, 0.f, 0.f}, ssq[4] = {0.f, 0.f, 0.f, 0.f};
  const int pxb0 = (wave * 32 + row16) * (STRIDE * CI);
  const int pxb1 = (wave * 32 + 16 + row16) * (STRIDE * CI);
  bf16* tw = ot + wave * 32 * OTROW;   // this wave's 32 px x 64 co tile
#pragma unroll 1
  for (int rr = 0; rr < rows; ++rr) {
    const int rshift = rr * STRIDE * XTROW;
    // one 16-px M-tile at a time (a real loop: 16 accumulators live, not
    // 32, so the weights stay in registers); each accumulator still sees
    // its five K-steps in the same order
#pragma unroll 1
    for (int m = 0; m < 2; ++m) {
      f32x4 acc[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = (f32x4)0.0f;
      const unsigned rb = 2u * (unsigned)(rshift + (m ? pxb1 : pxb0));
      const uint4* tp = reinterpret_cast<const uint4*>(ktab) + kgrp * 5;
      asm volatile("" : "+v"(tp));  // re-read per tile, do not hoist
#pragma unroll
      for (int kk = 0; kk < KPAD / 32; ++kk) {
        const uint4 t4 = tp[kk];
        const unsigned tk[4] = {t4.x, t4.y, t4.z, t4.w};
        bf16x8 f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int k = kk * 32 + kgrp * 8 + j;
          // K-padding taps read xt[0], row 0's lead pad: always zero
          const bool kz = (kk == KPAD / 32 - 1) && k >= KTAP;
          const unsigned pk = tk[j >> 1];
          const unsigned ob = ((j & 1) ? (pk >> 16) : (pk & 0xffffu)) + rb;
          f[j] = *reinterpret_cast<const bf16*>(
              reinterpret_cast<const char*>(xt) + (kz ? 0u : ob));
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
          acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              f, bfrag[kk][c], acc[c], 0, 0, 0);
      }
      // D col = lane&15 (co), row = 4*(lane>>4)+r (px): round, count
      // into the statistics, and transpose through the wave's tile
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int pxl = m * 16 + kgrp * 4 + r;
        const bool live = wave * 32 + pxl < WO;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const bf16 v = (bf16)acc[c][r];
          tw[pxl * OTROW + c * 16 + row16] = v;
          const float f = live ? (float)v : 0.f;
          ssum[c] += f;
          ssq[c] += f * f;
        }
      }
    }
    // the tile is wave-private and a wave's LDS operations complete in
    // order, so wave-scope ordering is all the hand-over needs
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const long long rowbase = ((long long)n * HO + ho0 + rr) * WO;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int v = lane + t * 64;
      const int pxl = v >> 3, j8 = (v & 7) * 8;
      const int px = wave * 32 + pxl;
      const bf16x8 val = *reinterpret_cast<const bf16x8*>(
          tw + pxl * OTROW + j8);
      if (px < WO)
        *reinterpret_cast<bf16x8*>(out + (rowbase + px) * CO + j8) = val;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }

  // statistics: the four px groups of a wave, then the four waves (fixed
  // order), then this block's slot
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    ssum[c] += __shfl_xor(ssum[c], 16, 64);
    ssum[c] += __shfl_xor(ssum[c], 32, 64);
    ssq[c] += __shfl_xor(ssq[c], 16, 64);
    ssq[c] += __shfl_xor(ssq[c], 32, 64);
  }
  float* red = reinterpret_cast<float*>(tw);  // own tile: reads are done
  if (kgrp == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      red[c * 16 + row16] = ssum[c];
      red[CO + c * 16 + row16] = ssq[c];
    }
  }
  __syncthreads();
  if (tid < 2 * CO) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w)
      t += reinterpret_cast<const float*>(ot + w * 32 * OTROW)[tid];
    partial[(long long)tid * gridDim.x + blockIdx.x] = t;
  }
}

// ------------------------------------------------- wrw (element gather)
// The first wrw kernel, kept selectable (MI355X_STEM_WRW_TR=0) for A/B
// runs and as a second implementation the tests compare against.
// block = 256 threads (4 waves) loops over ``rows_per_block`` output
// rows; per row: band stage + dy-row stage, then each wave reduces ALL
// four 32-px slices into its own (co, k) QUADRANT (2 co-subtiles x 5
// k-subtiles = 40 f32/lane; px-split waves would hold 160 accumulators
// and VGPR-cap occupancy at 1 wave/SIMD). A-frag = dy^T (row = co,
// k-slice = 8 px), B-frag gathered straight from the padded band.
// Partials atomic-add into the L2-resident [CO][KPAD] fp32 tile once
// per block (spread over 2.5k addresses — NOT the one-address-per-block
// serialization the round-1 notes warn about).
extern "C" __global__ __launch_bounds__(256) void stem_conv_wrw_gather_kernel(
    const bf16* __restrict__ x,    // [N][H][W][CI]
    const bf16* __restrict__ dy,   // [N][HO][WO][CO]
    float* __restrict__ dw,        // [CO][KPAD] fp32 (pre-zeroed)
    int Nb, int H, int W, int HO, int WO, int rows_per_block,
    int phase_mask) {
  __shared__ bf16 xt[8 * XTROW];
  __shared__ bf16 Dy[2 * PXPAD * CO];  // double-buffered dy row slices
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int row16 = lane & 15;
  const int kgrp = lane >> 4;
  const int nrows = Nb * HO;
  const int mw = (wave >> 1) * 2;   // this wave's co-subtiles: mw, mw+1
  const int cw = (wave & 1) * 5;    // this wave's k-subtiles: cw .. cw+4
  const int row_limit = min((blockIdx.x + 1) * rows_per_block, nrows);
  const int nch = (WO * CO) >> 3;
  const bf16x8 zv = {(bf16)0.0f, (bf16)0.0f, (bf16)0.0f, (bf16)0.0f,
                     (bf16)0.0f, (bf16)0.0f, (bf16)0.0f, (bf16)0.0f};

  f32x4 acc[2][5];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int c = 0; c < 5; ++c) acc[m][c] = (f32x4)0.0f;

  // dy is SOFTWARE-PIPELINED: row r+1's slice is loaded into registers
  // while row r's MFMA phase runs, and written to the other Dy buffer
  // after it — the per-row global-load stall (the largest wrw phase in
  // the ablation) hides under compute. Prologue: stage row 0 directly.
  int cur = 0;
  {
    const int row0 = blockIdx.x * rows_per_block;
    if (row0 < nrows) {
      const bf16x8* src = reinterpret_cast<const bf16x8*>(
          dy + (long long)row0 * WO * CO);
      bf16x8* d8 = reinterpret_cast<bf16x8*>(Dy);
      bf16x8 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = tid + u * 256;
        v[u] = (i < nch) ? src[i] : zv;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) d8[tid + u * 256] = v[u];
    }
  }

  for (int rr = 0; rr < rows_per_block; ++rr) {
    const int row = blockIdx.x * rows_per_block + rr;
    if (row >= nrows) break;
    const int n = row / HO;
    const int ho = row - n * HO;
    const bool prime = (rr == 0) || (ho == 0);
    __syncthreads();  // previous iteration's readers + Dy writes done
    if (prime)  // lead/tail pads must be zero before the first data rows
      for (int i = tid; i < 8 * XTROW; i += 256) xt[i] = (bf16)0.0f;
    __syncthreads();
    if (phase_mask & 1)
      stage_band_ring(x, xt, n, ho, H, W, tid, 256, prime);
    // prefetch NEXT row's dy slice (latency overlaps band stage,
    // barrier and the MFMA phase below)
    bf16x8 v[4];
    const bool have_next = (phase_mask & 2) && row + 1 < row_limit;
    if (have_next) {
      const bf16x8* src = reinterpret_cast<const bf16x8*>(
          dy + (long long)(row + 1) * WO * CO);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = tid + u * 256;
        v[u] = (i < nch) ? src[i] : zv;
      }
    }
    __syncthreads();
    if (phase_mask & 4) {
      // (MFMA phase reads Dy[cur], written one iteration ago)
    } else {
      if (have_next) {
        bf16x8* d8 = reinterpret_cast<bf16x8*>(Dy + (cur ^ 1) * PXPAD * CO);
#pragma unroll
        for (int u = 0; u < 4; ++u) d8[tid + u * 256] = v[u];
        cur ^= 1;
      }
      continue;
    }

#pragma unroll
    for (int sl = 0; sl < 4; ++sl) {
      const int pxbase = sl * 32;
      bf16x8 afrag[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        bf16x8 f;
        const bf16* dycur = Dy + cur * PXPAD * CO;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          f[j] = dycur[(pxbase + kgrp * 8 + j) * CO + (mw + m) * 16 + row16];
        afrag[m] = f;
      }
#pragma unroll
      for (int c = 0; c < 5; ++c) {
        const int k = (cw + c) * 16 + row16;
        const int kh = k / (KW * CI);
        const int r21 = k - kh * (KW * CI);
        // ring slot for this tap's input row; pad taps zero-selected
        const int ko = ((ho * STRIDE - PADDING + kh) & 7) * XTROW +
                       (XTOFF - PADDING * CI) + r21;
        const bool kz = k >= KTAP;
        bf16x8 bfr;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          bfr[j] = kz ? (bf16)0.0f
                      : xt[ko + (pxbase + kgrp * 8 + j) * (STRIDE * CI)];
#pragma unroll
        for (int m = 0; m < 2; ++m)
          acc[m][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              afrag[m], bfr, acc[m][c], 0, 0, 0);
      }
    }
    if (have_next) {
      bf16x8* d8 = reinterpret_cast<bf16x8*>(Dy + (cur ^ 1) * PXPAD * CO);
#pragma unroll
      for (int u = 0; u < 4; ++u) d8[tid + u * 256] = v[u];
      cur ^= 1;
    }
  }

  // D row = co (4*(lane>>4)+r), col = k (c*16 + lane&15)
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int c = 0; c < 5; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = (mw + m) * 16 + kgrp * 4 + r;
        const int k = (cw + c) * 16 + row16;
        atomicAdd(&dw[co * KPAD + k], acc[m][c][r]);
      }
}

// ------------------------------------------------ wrw (transposed reads)
// The contraction index of this GEMM is the pixel, and the pixel is the
// STRIDED index of both operands as they lie in LDS (dy is [px][co], the
// band is [px*6 + tap]), so the kernel above builds every MFMA operand
// from two-byte LDS reads: 56 of them plus packing per 10 MFMAs, and LDS
// instruction issue is what it waits on. ds_read_b64_tr_b16 reads a
// 4-row x 16-column block and hands each lane one column (4 K values in
// one 8-byte read). What that needs, and how it is met here:
//   * every lane address 8-byte aligned. Output pixels are 12 bytes apart
//     in the band, so (a) the wrw has its own tap order
//         k' = kh*24 + 3 + kw*3 + ci
//     (a pixel's 24-tap window starts one input pixel early, at iw =
//     2*px - 4, which is 8-byte aligned for even px; the three lead taps
//     per kernel row multiply a neighbouring real pixel, finite garbage
//     in dw columns the cast kernel never reads, so there is no
//     zero-select; the same goes for columns 168..175 of the last
//     tap-subtile, an eighth pseudo kernel row kh = 7: they read ring
//     slot (ih0+7)&7, which holds the prologue zeros or the input row
//     staged for the next output row, is in bounds and is only written
//     behind the barrier), and (b) there are two band images 4 bytes out of
//     phase: even pixels read the first, odd pixels the second;
//   * K is contracted, so any pixel -> K-slot map works as long as A and
//     B share it: K-group g (16 lanes) of read t takes the four pixels
//     8g + ((g+t)&1) + {0,2,4,6} of the 32-px slice: one parity per
//     block, and the eight dy rows one 32-lane half reads are distinct
//     mod 8, which with 160-byte dy rows is conflict-free;
//   * EXEC all ones at every transposed read: control flow around them is
//     block- or wave-uniform (scalar branches), tails are padded with
//     zeros (dy beyond WO) instead of masked.
// Wave split: 4 co-subtiles x 11 tap-subtiles (176 >= 168); wave w takes
// co-subtiles {2(w>>1), +1} and tap-subtiles 0..5 (w even) or 6..10 (w
// odd): per slice 4 + 12 (10) eight-byte reads for 12 (10) MFMAs.
// Row loop: the next row's dy slice AND its two new band rows are
// prefetched into registers before the MFMA phase and written after it,
// so a row costs one barrier pair; slices wholly beyond WO are skipped.
// LDS: 2 band images (26,112 B) + one dy row (20,480 B) = 46,592 B ->
// 3 blocks/CU, which the launch bounds also ask of the registers (154
// VGPRs, no scratch; the gather kernel's 224 allowed 2).
#define TRK 24                  // taps per kernel row in the wrw order
#define KPADT 176               // 7*24 = 168 -> 11 sixteen-tap subtiles
#define NKT (KPADT / 16)
#define DYROW 80                // dy row stride (els): 160 B
#define XTIMG (8 * XTROW)       // one band image (8 ring slots)
#define XTODD (XTIMG + 2)       // odd-pixel image: same data, +4 bytes

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
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

// four band elements (chunk c of a row) into ring slot ``slot`` of both
// images; the shifted image is only 4-byte aligned
__device__ __forceinline__ void band_put(bf16* xt, int slot, int c,
                                         bf16x4 v) {
  bf16* e = xt + slot * XTROW + XTOFF + 4 * c;
  *reinterpret_cast<bf16x4*>(e) = v;
  const bf16x2 lo = {v[0], v[1]}, hi = {v[2], v[3]};
  *reinterpret_cast<bf16x2*>(e + XTODD) = lo;
  *reinterpret_cast<bf16x2*>(e + XTODD + 2) = hi;
}

// Stage input rows rfirst..6 of output row (n, ho) into their ring slots
// (slot = ih & 7) of both images, zeros for rows outside the image.
// Not pipelined: used for a block's first row, at image boundaries and
// for row lengths that are no multiple of 4 elements.
__device__ __forceinline__ void wrw_stage_rows(
    const bf16* __restrict__ x, bf16* xt, int n, int ho, int rfirst,
    int H, int W, int tid) {
  const int rowlen = W * CI;
  const int ih0 = ho * STRIDE - PADDING;
  if ((rowlen & 3) == 0) {
    const int nch = rowlen >> 2;
    const int total = (KH - rfirst) * nch;
    const bf16x4 z = {(bf16)0.0f, (bf16)0.0f, (bf16)0.0f, (bf16)0.0f};
    for (int base = 0; base < total; base += 256 * 4) {
      bf16x4 v[4];
      int ss[4], cc[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = base + tid + u * 256;
        v[u] = z;
        ss[u] = -1;
        if (i < total) {
          const int r = i / nch, c = i - r * nch;
          const int ih = ih0 + rfirst + r;
          ss[u] = ih & 7; cc[u] = c;
          if (ih >= 0 && ih < H)
            v[u] = reinterpret_cast<const bf16x4*>(
                x + ((long long)n * H + ih) * rowlen)[c];
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (ss[u] >= 0) band_put(xt, ss[u], cc[u], v[u]);
    }
  } else {
    for (int r = rfirst; r < KH; ++r) {
      const int ih = ih0 + r;
      const bool in = ih >= 0 && ih < H;
      const bf16* src = x + ((long long)n * H + (in ? ih : 0)) * rowlen;
      bf16* dst = xt + (ih & 7) * XTROW + XTOFF;
      for (int i = tid; i < rowlen; i += 256) {
        const bf16 v = in ? src[i] : (bf16)0.0f;
        dst[i] = v;
        dst[i + XTODD] = v;
      }
    }
  }
}

extern "C" __global__ __launch_bounds__(256, 3) void stem_conv_wrw_kernel(
    const bf16* __restrict__ x,    // [N][H][W][CI]
    const bf16* __restrict__ dy,   // [N][HO][WO][CO]
    float* __restrict__ dw,        // [CO][KPADT] fp32 (pre-zeroed), k' order
    int Nb, int H, int W, int HO, int WO, int rows_per_block,
    int phase_mask) {
  __shared__ __attribute__((aligned(16))) bf16 xt[2 * XTIMG];
  __shared__ __attribute__((aligned(16))) bf16 Dy[PXPAD * DYROW];
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int l16 = lane & 15;
  const int kgrp = lane >> 4;
  const int q = l16 >> 2, p = l16 & 3;  // block row / 4-column group
  const int nrows = Nb * HO;
  const int mw = (wave >> 1) * 2;       // co-subtiles mw, mw+1
  const int cw = (wave & 1) * 6;        // tap-subtiles cw .. cw+nk-1
  const int nk = min(6, NKT - cw);
  const int row0 = blockIdx.x * rows_per_block;
  const int row_limit = min(row0 + rows_per_block, nrows);
  if (row0 >= nrows) return;
  const int rowlen = W * CI;
  const bool vec = (rowlen & 3) == 0;
  const int nchx = rowlen >> 2;         // 8-byte chunks per input row
  const int nch = (WO * CO) >> 3;       // 16-byte chunks per dy row
  const bf16x8 zv = {(bf16)0.0f, (bf16)0.0f, (bf16)0.0f, (bf16)0.0f,
                     (bf16)0.0f, (bf16)0.0f, (bf16)0.0f, (bf16)0.0f};
  const bf16x4 zx = {(bf16)0.0f, (bf16)0.0f, (bf16)0.0f, (bf16)0.0f};

  f32x4 acc[2][6];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int c = 0; c < 6; ++c) acc[m][c] = (f32x4)0.0f;

  // per-lane operand addressing. Read t (0/1) of K-group kgrp covers
  // pixels 8*kgrp + ((kgrp+t)&1) + 2*q' (q' = 0..3); this lane supplies
  // row q of the block, columns 4p..4p+3.
  int aoff[2], boffpx[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int par = (kgrp + t) & 1;
    const int px = 8 * kgrp + par + 2 * q;
    aoff[t] = px * DYROW + mw * 16 + 4 * p;
    boffpx[t] = par * XTODD + px * (STRIDE * CI);
  }
  // tap-subtile c of this wave, columns 4p..4p+3: kernel row and offset
  int khc[6], rc[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    const int kq = (cw + c) * 16 + 4 * p;
    khc[c] = kq / TRK;
    rc[c] = kq - khc[c] * TRK;
  }

  // prologue: zero both images (pads stay zero for the whole block: the
  // data region is overwritten with the same W every row), dy row 0
  for (int i = tid; i < 2 * XTIMG / 8; i += 256)
    reinterpret_cast<bf16x8*>(xt)[i] = zv;
  {
    const bf16x8* src = reinterpret_cast<const bf16x8*>(
        dy + (long long)row0 * WO * CO);
    bf16x8 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = tid + u * 256;
      v[u] = (i < nch) ? src[i] : zv;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = tid + u * 256;
      *reinterpret_cast<bf16x8*>(Dy + (i >> 3) * DYROW + (i & 7) * 8) = v[u];
    }
  }
  __syncthreads();
  if (phase_mask & 1)
    wrw_stage_rows(x, xt, row0 / HO, row0 % HO, 0, H, W, tid);
  __syncthreads();

  int n = row0 / HO;
  int ho = row0 - n * HO;
  for (int row = row0; row < row_limit; ++row) {
    const bool have_next = row + 1 < row_limit;
    const bool next_same = have_next && ho + 1 < HO;  // same image
    // prefetch the next row's dy slice and (ring band) its two new input
    // rows; the latency hides under the MFMA phase
    bf16x8 v[4];
    bf16x4 bv[2];
    if (have_next && (phase_mask & 2)) {
      const bf16x8* src = reinterpret_cast<const bf16x8*>(
          dy + (long long)(row + 1) * WO * CO);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = tid + u * 256;
        v[u] = (i < nch) ? src[i] : zv;
      }
    }
    const int ihn = (ho + 1) * STRIDE - PADDING + (KH - STRIDE);
    if (next_same && vec && (phase_mask & 1)) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int i = tid + u * 256;
        const int r = i >= nchx ? 1 : 0;
        const int c = i - r * nchx;
        bv[u] = zx;
        if (c < nchx && ihn + r < H)
          bv[u] = reinterpret_cast<const bf16x4*>(
              x + ((long long)n * H + ihn + r) * rowlen)[c];
      }
    }

    if (phase_mask & 4) {
      const int ih0 = ho * STRIDE - PADDING;
      int boff[6];
#pragma unroll
      for (int c = 0; c < 6; ++c)
        boff[c] = ((ih0 + khc[c]) & 7) * XTROW + rc[c];
#pragma unroll
      for (int sl = 0; sl < 4; ++sl) {
        if (sl * 32 >= WO) break;  // block-uniform
        bf16x8 af[2];
#pragma unroll
        for (int m = 0; m < 2; ++m)
          af[m] = tr_frag(Dy + aoff[0] + sl * 32 * DYROW + m * 16,
                          Dy + aoff[1] + sl * 32 * DYROW + m * 16);
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          if (c < nk) {  // wave-uniform
            const int so = sl * 32 * STRIDE * CI;
            const bf16x8 bfr = tr_frag(xt + boff[c] + boffpx[0] + so,
                                       xt + boff[c] + boffpx[1] + so);
#pragma unroll
            for (int m = 0; m < 2; ++m)
              acc[m][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  af[m], bfr, acc[m][c], 0, 0, 0);
          }
        }
      }
    }
    if (!have_next) break;

    __syncthreads();  // every wave is done reading this row's operands
    if (phase_mask & 2) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = tid + u * 256;
        *reinterpret_cast<bf16x8*>(Dy + (i >> 3) * DYROW + (i & 7) * 8) =
            v[u];
      }
    }
    if (phase_mask & 1) {
      if (!next_same) {
        wrw_stage_rows(x, xt, n + 1, 0, 0, H, W, tid);
      } else if (!vec) {
        wrw_stage_rows(x, xt, n, ho + 1, KH - STRIDE, H, W, tid);
      } else {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int i = tid + u * 256;
          const int r = i >= nchx ? 1 : 0;
          const int c = i - r * nchx;
          if (c < nchx) band_put(xt, (ihn + r) & 7, c, bv[u]);
        }
      }
    }
    __syncthreads();
    if (++ho == HO) { ho = 0; ++n; }
  }

  // D row = co (4*(lane>>4)+r), col = k' (c*16 + lane&15)
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int c = 0; c < 6; ++c)
      if (c < nk) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int co = (mw + m) * 16 + kgrp * 4 + r;
          const int k = (cw + c) * 16 + l16;
          atomicAdd(&dw[co * KPADT + k], acc[m][c][r]);
        }
      }
}

// dw fp32 -> bf16 grad in the conv weight's layout [CO][KTAP]; ``tr``:
// dw is [CO][KPADT] in the transposed-read kernel's tap order k',
// otherwise [CO][KPAD] in weight order
extern "C" __global__ __launch_bounds__(256) void stem_wrw_cast_kernel(
    const float* __restrict__ dw, bf16* __restrict__ out, int tr) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < CO * KTAP) {
    const int co = i / KTAP, k = i - co * KTAP;
    const int kh = k / (KW * CI);
    out[i] = (bf16)(tr ? dw[co * KPADT + k + kh * (TRK - KW * CI) + 3]
                       : dw[co * KPAD + k]);
  }
}

// Blocks (= statistics slots per channel) of the fused-statistics forward.
extern "C" int stem_fwd_stat_blocks(int Nb, int HO) {
  return Nb * ((HO + FWD_ROWS - 1) / FWD_ROWS);
}

// ``partial`` null: the one-row-per-block kernel, no statistics (the BN
// reduce then reads the map back). Non-null: fp32 [2*CO][
// stem_fwd_stat_blocks] scratch, filled with the per-block channel sums.
extern "C" void launch_stem_conv_fwd(const void* x, const void* w, void* out,
                                     void* wp_scratch, float* partial,
                                     int Nb, int H, int W, int HO, int WO,
                                     hipStream_t stream, int phase_mask) {
  hipLaunchKernelGGL(stem_pad_weights_kernel,
                     dim3((CO * KPAD + 255) / 256), dim3(256), 0, stream,
                     (const bf16*)w, (bf16*)wp_scratch);
  if (partial) {
    const int nchunks = (HO + FWD_ROWS - 1) / FWD_ROWS;
    hipLaunchKernelGGL(stem_conv_fwd_stats_kernel, dim3(Nb * nchunks),
                       dim3(256), 0, stream, (const bf16*)x,
                       (const bf16*)wp_scratch, (bf16*)out, partial,
                       Nb, H, W, HO, WO, nchunks, phase_mask);
    return;
  }
  hipLaunchKernelGGL(stem_conv_fwd_kernel, dim3(Nb * HO), dim3(256), 0,
                     stream, (const bf16*)x, (const bf16*)wp_scratch,
                     (bf16*)out, Nb, H, W, HO, WO, phase_mask);
}

extern "C" void launch_stem_conv_wrw(const void* x, const void* dy,
                                     float* dw_f32, void* dw_bf16,
                                     int Nb, int H, int W, int HO, int WO,
                                     hipStream_t stream,
                                     int phase_mask, int tr) {
  const int nrows = Nb * HO;
  const int target_blocks = 768;
  const int rpb = (nrows + target_blocks - 1) / target_blocks;
  const int blocks = (nrows + rpb - 1) / rpb;
  (void)hipMemsetAsync(dw_f32, 0, CO * KPADT * sizeof(float), stream);
  if (tr)
    hipLaunchKernelGGL(stem_conv_wrw_kernel, dim3(blocks), dim3(256), 0,
                       stream, (const bf16*)x, (const bf16*)dy, dw_f32,
                       Nb, H, W, HO, WO, rpb, phase_mask);
  else
    hipLaunchKernelGGL(stem_conv_wrw_gather_kernel, dim3(blocks), dim3(256),
                       0, stream, (const bf16*)x, (const bf16*)dy, dw_f32,
                       Nb, H, W, HO, WO, rpb, phase_mask);
  hipLaunchKernelGGL(stem_wrw_cast_kernel,
                     dim3((CO * KTAP + 255) / 256), dim3(256), 0, stream,
                     dw_f32, (bf16*)dw_bf16, tr);
}

// fp32 elements of the wrw accumulation scratch (either kernel)
extern "C" int stem_wrw_scratch_elems() { return CO * KPADT; }
