// Hand-written MFMA 3x3 / stride 1 / pad 1 convolution for gfx950, NHWC
// bf16: forward, forward with BatchNorm statistics in the epilogue, and
// (through a weight repack) data-grad. One kernel template serves every
// shape: Cin, Cout multiples of 64, 1 <= W <= 64, any H and N.
//
// Why: sixteen of ResNet-18's twenty convs are 3x3 / s1 / p1, each followed
// by a BN whose reduce pass re-reads the whole output only to sum it.
//
//   Y[n,h,w,co] = sum_{kh,kw,ci} X[n,h+kh-1,w+kw-1,ci] * Wt[co,kh,kw,ci]
//
// An implicit GEMM on v_mfma_f32_16x16x32_bf16 with fp32 accumulation. A
// channels-last weight [Cout,Cin,3,3] lies as [Cout][3][3][Cin]: every
// output channel owns one contiguous K = 9*Cin row in (kh, kw, ci) order,
// so the B operand is staged as conv1x1_gemm_kernel stages its own (64 co
// x 64 ci tiles, 16-byte loads along ci). The A operand is what differs:
//
//   * padded-flat coordinates. The input is seen as a virtual zero-bordered
//     map [N][H+2][W+2] with flat index q = (n*(H+2) + h+1)*(W+2) + w+1. A
//     block owns 128 consecutive q and 64 output channels (the pointwise
//     kernel's work split: 256 threads, a wave 32 rows x 64 columns = 2 x 4
//     accumulator tiles, column tiles of one M-block adjacent in launch
//     order so the band comes from HBM once and from L2 afterwards). In
//     these coordinates a tap is ONE constant offset, (kh-1)*(W+2) +
//     (kw-1): the main loop has no division and no bounds test, and a
//     lane's A address is the tap's row offset plus the XOR swizzle of that
//     row. Outputs that fall on border positions are computed and thrown
//     away; the useful share of the MFMAs is H*W / ((H+2)*(W+2)): 93 % at
//     56, 87 % at 28, 77 % at 14, 60 % at 7.
//   * band staging. For each 64-channel chunk of Cin the block stages ONE
//     band: virtual pixels q0-(W+3) .. q0+127+(W+3), 128 + 2W + 6 rows of
//     128 bytes, global -> registers -> LDS with 16-byte accesses and the
//     pointwise kernel's swizzle (chunk ^ (row & 7)). That band feeds all
//     nine taps: tap (kh, kw) reads band row local_q + kh*(W+2) + kw. No
//     im2col, no per-tap gather. Each staged row's real pixel (or "zero":
//     border rows and rows outside [0, N*(H+2)*(W+2))) is found ONCE per
//     block before the K loop, by two mul-hi divisions with host-computed
//     reciprocals (as s2_divmod in conv1x1.hip); the loop only multiplies
//     the pixel by Cin.
//   * pipeline. K runs chunk-major, tap-minor. Weight tiles (8 KB) are
//     double-buffered: the loads of step s+1 are issued before the MFMAs of
//     step s and stored after them, one barrier per step. The band is
//     single-buffered: the next chunk's band is loaded into registers (nine
//     16-byte loads per thread at most) under taps 6..8 and stored behind
//     one extra barrier per chunk.
//   * LDS is sized from W at launch: 16 KB of weight tiles + the band,
//     49,920 bytes at W = 64 (262 rows), 32,512 at W = 56: three blocks per
//     CU for every shape.
//   * epilogue, as the pointwise kernel's: round to bf16, transpose through
//     a wave-private LDS tile, 16-byte stores along the channel axis. One
//     lane per tile row maps its q to a pixel (or "border") once; the store
//     loop and the statistics fetch that by shuffle / ballot. Only real
//     pixels are stored. Statistics: border rows are forced to zero, then
//     each lane sums value and square of the ROUNDED outputs, lanes add by
//     shuffle, waves through LDS in a fixed order, one thread per column
//     writes slot [channel][M-block] of the [2*Cout][nblocks] partials,
//     nblocks = ceil(N*(H+2)*(W+2) / 128). No atomics: bit-reproducible.
//
// Data-grad: for stride 1 / pad 1, dX is the same convolution applied to dY
// with the weight rotated and transposed, Wf[ci][kh][kw][co] =
// Wt[co][2-kh][2-kw][ci]. conv3x3_wflip_kernel writes Wf (at most 4.7 MB,
// 64 x 64 tiles through LDS, 16-byte accesses on both sides) and the
// forward kernel runs on it: there is no second GEMM body.
//
// Compiler resource usage (hipcc -O3, gfx950): conv3x3_fwd_kernel 152 VGPRs
// with and without statistics (budget for three blocks per CU: 168), LDS
// dynamic as above (at most 49,920 B; budget 53 KB), 3 waves per SIMD = 3
// blocks per CU; conv3x3_wflip_kernel 22 VGPRs, 9,216 B LDS, 8 waves per
// SIMD. Scratch is 0 for all three.
#include <hip/hip_runtime.h>
#include "conv_mfma.h"

#define C3_BM 128               // virtual pixels per block
#define C3_BN 64                // output channels per block
#define C3_BK 64                // channels per Cin chunk
#define C3_OTROW 72             // epilogue tile row stride (els): 144 B
#define C3_MAXU 9               // 32-row staging passes: ceil(262 / 32)

// element offset of 16-byte chunk ``ch`` of row ``row`` in a [rows][64] tile
__device__ __forceinline__ int c3_swz(int row, int ch) {
  return row * C3_BK + ((ch ^ (row & 7)) << 3);
}

// Y[pixel][Cout] over the virtual pixels, Wt = [Cout][9][Cin]. grid =
// ceil(Q / 128) * (Cout / 64), column tiles fastest; dynamic LDS =
// conv3x3_lds_bytes(W). phase_mask: 1 = global loads + LDS staging, 4 =
// MFMA, 2 = epilogue.
template <bool STATS>
__global__ __launch_bounds__(256, 3) void conv3x3_fwd_kernel(
    const bf16* __restrict__ X, const bf16* __restrict__ Wt,
    bf16* __restrict__ Y,
    float* __restrict__ partial,  // [2*Cout][ceil(Q / 128)], STATS only
    int Cin, int Cout, int ntn, int phase_mask, const C3Geo g) {
  extern __shared__ __attribute__((aligned(16))) bf16 smem[];
  bf16* const Bs = smem;                      // [2][64 co][64 ci]
  bf16* const As = smem + 2 * C3_BN * C3_BK;  // band [128 + 2W + 6][64 ci]
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int l16 = lane & 15;
  const int kgrp = lane >> 4;
  const int mb = blockIdx.x / ntn;
  const int nb = blockIdx.x - mb * ntn;
  const int q0 = mb * C3_BM, n0 = nb * C3_BN;
  const int nmb = gridDim.x / ntn;
  const int brows = C3_BM + 2 * g.Wp + 2;  // band rows

  // staging: thread -> 16-byte chunk (tid & 7) of rows (tid >> 3) + 32u;
  // the swizzle term is the same for every u (32u is a multiple of 8)
  const int srow = tid >> 3, sch = tid & 7;
  const int sto = c3_swz(srow, sch);
  // band row b is virtual pixel q0 - (W+3) + b: its real pixel, -1 = a row
  // of zeros, -2 = beyond the band (nothing staged)
  int pix[C3_MAXU];
#pragma unroll
  for (int u = 0; u < C3_MAXU; ++u) {
    const int b = srow + 32 * u;
    pix[u] = b < brows ? c3_pixel((long long)q0 - (g.Wp + 1) + b, g) : -2;
  }
  const bf16* const pa = X + sch * 8;
  const bf16* const pb = Wt + ((long long)n0 + srow) * 9 * Cin + sch * 8;
  const int bstep = 32 * 9 * Cin;  // 32 weight rows
  const bf16x8 zv = {(bf16)0.0f, (bf16)0.0f, (bf16)0.0f, (bf16)0.0f,
                     (bf16)0.0f, (bf16)0.0f, (bf16)0.0f, (bf16)0.0f};

  // operand addressing: B as the pointwise kernel; an A row moves with the
  // tap, so its swizzle term is taken per tap
  const int bsw = l16 & 7;
  const int bo0 = l16 * C3_BK + ((kgrp ^ bsw) << 3);  // K 0..31
  const int bo1 = bo0 ^ 32;                           // K 32..63
  const int arow = wave * 32 + l16;

  f32x4 acc[2][4];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[m][c] = (f32x4)0.0f;

  bf16x8 ra[C3_MAXU], rb[2];

#define C3_BAND_LOAD(cof)                                                   \
  {                                                                         \
    _Pragma("unroll") for (int u = 0; u < C3_MAXU; ++u)                     \
      ra[u] = pix[u] >= 0 ? *reinterpret_cast<const bf16x8*>(               \
                                pa + (long long)pix[u] * Cin + (cof))       \
                          : zv;                                             \
  }
#define C3_BAND_STORE()                                                     \
  {                                                                         \
    _Pragma("unroll") for (int u = 0; u < C3_MAXU; ++u)                     \
      if (pix[u] != -2)                                                     \
        *reinterpret_cast<bf16x8*>(As + sto + u * 32 * C3_BK) = ra[u];      \
  }
#define C3_W_LOAD(kof)                                                      \
  {                                                                         \
    _Pragma("unroll") for (int u = 0; u < 2; ++u)                           \
      rb[u] = *reinterpret_cast<const bf16x8*>(pb + u * bstep + (kof));     \
  }
#define C3_W_STORE(buf)                                                     \
  {                                                                         \
    _Pragma("unroll") for (int u = 0; u < 2; ++u)                           \
      *reinterpret_cast<bf16x8*>(Bs + (buf) * C3_BN * C3_BK + sto +         \
                                 u * 32 * C3_BK) = rb[u];                   \
  }

  if (phase_mask & 1) {
    C3_BAND_LOAD(0)
    C3_W_LOAD(0)
    C3_BAND_STORE()
    C3_W_STORE(0)
  }
  __syncthreads();

  const int nch = Cin / C3_BK;
#pragma unroll 1
  for (int c = 0; c < nch; ++c) {
    const bool nextc = c + 1 < nch;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int buf = (c + t) & 1;  // parity of step 9c + t
      const bool more = t < 8 || nextc;
      if (more && (phase_mask & 1)) {
        if (t < 8) C3_W_LOAD((t + 1) * Cin + c * C3_BK)
        else C3_W_LOAD((c + 1) * C3_BK)
      }
      if (t == 6 && nextc && (phase_mask & 1)) C3_BAND_LOAD((c + 1) * C3_BK)
      if (phase_mask & 4) {
        const bf16* bs = Bs + buf * C3_BN * C3_BK;
        const int r0 = arow + (t / 3) * g.Wp + (t % 3);  // band row, m = 0
        const int ao = r0 * C3_BK, asw = r0 & 7;         // r0 + 16: same & 7
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          const int fa = ((4 * kk + kgrp) ^ asw) << 3;
          bf16x8 af[2], bfr[4];
#pragma unroll
          for (int m = 0; m < 2; ++m)
            af[m] = *reinterpret_cast<const bf16x8*>(
                As + ao + m * 16 * C3_BK + fa);
#pragma unroll
          for (int cc = 0; cc < 4; ++cc)
            bfr[cc] = *reinterpret_cast<const bf16x8*>(
                bs + cc * 16 * C3_BK + (kk ? bo1 : bo0));
#pragma unroll
          for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int cc = 0; cc < 4; ++cc)
              acc[m][cc] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  af[m], bfr[cc], acc[m][cc], 0, 0, 0);
        }
      }
      if (t == 8 && nextc) {
        __syncthreads();  // every wave is done with this chunk's band
        if (phase_mask & 1) C3_BAND_STORE()
      }
      if (more && (phase_mask & 1)) C3_W_STORE(buf ^ 1)
      __syncthreads();  // step s is read, step s+1 is in place
    }
  }
#undef C3_BAND_LOAD
#undef C3_BAND_STORE
#undef C3_W_LOAD
#undef C3_W_STORE
  if (!(phase_mask & 2)) return;

  // lanes l and l + 32 map row (l & 31) of the wave's 32 to its pixel
  const int opix = c3_pixel((long long)q0 + wave * 32 + (lane & 31), g);
  const unsigned real = (unsigned)__ballot(opix >= 0);  // bit r: row r is real

  // D col = lane&15, row = 4*(lane>>4)+r: round, count into the
  // statistics, and transpose through the wave's own tile (the operand
  // buffers are free behind the loop's last barrier)
  bf16* tw = smem + wave * 32 * C3_OTROW;
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
        tw[row * C3_OTROW + c * 16 + l16] = v;
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
        *reinterpret_cast<const bf16x8*>(tw + rl * C3_OTROW + j8);
    if (p >= 0)
      *reinterpret_cast<bf16x8*>(Y + (long long)p * Cout + n0 + j8) = val;
  }

  if (STATS) {
    // the four row groups of a wave, then the four waves (fixed order),
    // then this M-block's slot of the block's 64 columns
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      ssum[c] += __shfl_xor(ssum[c], 16, 64);
      ssum[c] += __shfl_xor(ssum[c], 32, 64);
      ssq[c] += __shfl_xor(ssq[c], 16, 64);
      ssq[c] += __shfl_xor(ssq[c], 32, 64);
    }
    float* red = reinterpret_cast<float*>(smem + 4 * 32 * C3_OTROW);
    if (kgrp == 0) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        red[wave * 2 * C3_BN + c * 16 + l16] = ssum[c];
        red[wave * 2 * C3_BN + C3_BN + c * 16 + l16] = ssq[c];
      }
    }
    __syncthreads();
    if (tid < 2 * C3_BN) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) s += red[w * 2 * C3_BN + tid];
      const int ch = tid < C3_BN ? n0 + tid : Cout + n0 + tid - C3_BN;
      partial[(long long)ch * nmb + mb] = s;
    }
  }
}

// Wf[ci][t][co] = Wt[co][8 - t][ci], t = 3*kh + kw: the data-grad's weight.
// grid = (Cin / 64, Cout / 64, 9); a block turns one 64 x 64 tile over.
__global__ __launch_bounds__(256) void conv3x3_wflip_kernel(
    const bf16* __restrict__ Wt, bf16* __restrict__ Wf, int Cin, int Cout) {
  __shared__ __attribute__((aligned(16))) bf16 tile[64 * C3_OTROW];
  const int tid = threadIdx.x;
  const int row = tid >> 3, ch = tid & 7;
  const int ci0 = blockIdx.x * 64, co0 = blockIdx.y * 64, t = blockIdx.z;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int co = row + 32 * u;
    *reinterpret_cast<bf16x8*>(tile + co * C3_OTROW + ch * 8) =
        *reinterpret_cast<const bf16x8*>(
            Wt + ((long long)(co0 + co) * 9 + (8 - t)) * Cin + ci0 + ch * 8);
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int ci = row + 32 * u;
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = tile[(ch * 8 + j) * C3_OTROW + ci];
    *reinterpret_cast<bf16x8*>(
        Wf + ((long long)(ci0 + ci) * 9 + t) * Cout + co0 + ch * 8) = o;
  }
}

// M-blocks (= statistics slots per channel): ceil(N*(H+2)*(W+2) / 128)
extern "C" int conv3x3_m_blocks(long long N, long long H, long long W) {
  return (int)((N * (H + 2) * (W + 2) + C3_BM - 1) / C3_BM);
}

// weight tiles + band, in bytes
static size_t conv3x3_lds_bytes(int W) {
  return (size_t)(2 * C3_BN + C3_BM + 2 * W + 6) * C3_BK * sizeof(bf16);
}

// x [N,H,W,Cin], w [Cout,3,3,Cin], out [N,H,W,Cout]. ``partial`` null: no
// statistics. Non-null: fp32 [2*Cout][conv3x3_m_blocks(N, H, W)].
extern "C" void launch_conv3x3_fwd(const void* x, const void* w, void* out,
                                   float* partial, int N, int H, int W,
                                   int Cin, int Cout, hipStream_t stream,
                                   int phase_mask) {
  const C3Geo g = c3_geo(N, H, W);
  const int ntn = Cout / C3_BN;
  const dim3 grid(conv3x3_m_blocks(N, H, W) * ntn), block(256);
  const size_t lds = conv3x3_lds_bytes(W);
  if (partial)
    hipLaunchKernelGGL(conv3x3_fwd_kernel<true>, grid, block, lds, stream,
                       (const bf16*)x, (const bf16*)w, (bf16*)out, partial,
                       Cin, Cout, ntn, phase_mask, g);
  else
    hipLaunchKernelGGL(conv3x3_fwd_kernel<false>, grid, block, lds, stream,
                       (const bf16*)x, (const bf16*)w, (bf16*)out,
                       (float*)nullptr, Cin, Cout, ntn, phase_mask, g);
}

// wf [Cin,3,3,Cout] from w [Cout,3,3,Cin]
extern "C" void launch_conv3x3_wflip(const void* w, void* wf, int Cin,
                                     int Cout, hipStream_t stream) {
  hipLaunchKernelGGL(conv3x3_wflip_kernel, dim3(Cin / 64, Cout / 64, 9),
                     dim3(256), 0, stream, (const bf16*)w, (bf16*)wf, Cin,
                     Cout);
}
