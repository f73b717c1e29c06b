// Weight-grad of the 3x3 / stride 1 / pad 1 conv with Cin == Cout == C (a
// multiple of 64 up to 2048), 1 <= W <= 64, any H and N, NHWC bf16, fp32
// accumulation: a split-K MFMA kernel in padded-flat coordinates.
//
//   dW[co][kh][kw][ci] = sum_q dYv[q][co] * Xv[q + (kh-1)(W+2) + (kw-1)][ci]
//
// q runs over the virtual pixels [0, Q), Q = N(H+2)(W+2), of the
// zero-bordered maps Xv and dYv (conv_mfma.h, as conv3x3.hip's forward).
// Zero rows of dYv make a border q contribute nothing; zero rows of Xv are
// the padding. There are no rows, no per-row phases and no K padding: a
// 32-pixel K-step simply spans rows and images, and the only waste is the
// border share of q (7 % at 56, 40 % at 7).
//
//   * work split: conv1x1_wrw_kernel's. 256 threads own a 64 co x 64 ci
//     tile of dW for ALL NINE taps and one chunk of K-steps; blockIdx.x =
//     chunk * tiles + tile, so the tiles of a chunk are neighbours in launch
//     order and a chunk's rows come from HBM once. A wave holds 16 ci x 64
//     co x 9 taps = 36 f32x4 accumulators (144 registers). The MFMA computes
//     dW^T: A = X^T (row = ci), B = dY (col = co). A lane then holds four
//     consecutive ci of one (co, tap): the epilogue is plain 16-byte stores into part[chunk][co][tap][ci], the
//     physical layout of a channels-last [C,C,3,3] weight. Every slot is
//     written by exactly one block: no atomics, bit-reproducible.
//   * operands. Per K-step the block stages the step's 32 rows of dY (zeros
//     where c3_pixel says border or beyond Q) into a double-buffered
//     [32][64] panel and 32 NEW rows of X into a ring of 256 rows x 128 B:
//     ring row r & 255 holds virtual pixel q0 - (W+3) + r, q0 the chunk's
//     first pixel. A step reads rows [32s, 32s + 32 + 2W + 6) while rows
//     [32(s+1) + 2W + 6, 32(s+2) + 2W + 6) are stored for the next one: a
//     span of 64 + 2W + 6 <= 198 rows, so nothing read is overwritten. A
//     block reads each X row once plus one halo of 2W + 6 rows per chunk
//     (the prologue). The loads of step s+1 are issued before the MFMAs of
//     step s and stored after them; one barrier per step. The q -> pixel map
//     is two mul-hi divisions per staged row; the loop has no other division.
//   * fragments: both operands come out of LDS with ds_read_b64_tr_b16
//     (tr_frag), from panels staged exactly as they lie in memory. Tap (kh,
//     kw) reads the ring at row local_q + kh(W+2) + kw; a transposed read
//     takes a per-lane address, so the offset is free, and the swizzle term
//     (wswz) is taken from the actual ring row. One dY fragment pair serves
//     all nine taps. EXEC is all ones at every transposed read: tails are
//     masked at the global loads only, and every ring row a step reads has
//     been stored (data or zeros), so a zero dY row never meets garbage.
//   * chunks: conv1x1_wrw_chunks' rule, about two blocks per CU of the
//     current device, with chunks of at least W3_MIN_STEPS = 8 K-steps: the
//     halo is up to 4.2 steps' worth of rows, so shorter chunks would stage
//     more halo than data. A request overrides the rule.
//   * reduce: conv1x1_wrw_reduce_kernel (conv1x1.hip) over the flat 9C^2
//     elements; stores bf16 or adds into the bf16 values present as a bf16
//     tensor add of the rounded result would. It is launched whatever the
//     phase mask, as in the pointwise weight-grad.
//
// Measured deviation from the first design (waves 2 x 2, a 32 x 32 quadrant
// each, ring addresses computed per read): that wave reads 18 X + 2 dY
// fragments per step and spends ~10 VALU instructions on every read's
// address; its MFMA phase alone took 77-109 us on the four ResNet-18 shapes
// at batch 212 and the call lost to MIOpen on two of them. With 16 ci x 64 co
// per wave a wave reads 9 X + 4 dY fragments for the same 36 MFMAs, and the
// ring offsets are loop-invariant up to one add and one mask (below): MFMA
// phase 55-72 us, call 85-109 us, faster than MIOpen + add on all four
// (BASELINE.md).
//
// Compiler resource usage (hipcc -O3, gfx950,
// -Rpass-analysis=kernel-resource-usage): conv3x3_wrw_kernel 226 VGPRs, 0
// AGPRs, 40,960 B LDS, scratch 0, no spills, 2 waves per SIMD = 2 blocks per
// CU (what __launch_bounds__(256, 2) asks for).
#include <hip/hip_runtime.h>
#include "conv_mfma.h"

#define W3_K 32                 // virtual pixels per K-step
#define W3_PANEL (W3_K * 64)    // elements of one [32][64] panel
#define W3_RING 256             // ring rows, a power of two >= 64 + 2*64 + 6
#define W3_PRO 6                // 32-row prologue passes: ceil(166 / 32)
#define W3_MIN_STEPS 8          // shortest chunk the default rule makes

extern "C" void launch_conv_wrw_reduce(const float* part, void* dw,
                                       long long nel, int nchunks,
                                       int accumulate, hipStream_t stream);

// element offset a transposed read hands in: row ``row`` of a panel,
// columns col0 + 4p .. 4p+3 (col0 a multiple of 16)
__device__ __forceinline__ int w3_tro(int row, int col0, int p) {
  return wswz(row, (col0 >> 3) + (p >> 1)) + (p & 1) * 4;
}

// part[chunk][C][9][C] = sum over the chunk's virtual pixels. grid = chunks
// * tiles; spc = K-steps per chunk (the last chunk may be shorter, never
// empty), steps = ceil(Q / 32). phase_mask: 1 = global loads + LDS staging,
// 4 = fragment reads + MFMA, 2 = epilogue.
__global__ __launch_bounds__(256, 2) void conv3x3_wrw_kernel(
    const bf16* __restrict__ X, const bf16* __restrict__ dY,
    float* __restrict__ part, int C, int nt, int tiles, int spc, int steps,
    int phase_mask, const C3Geo g) {
  __shared__ __attribute__((aligned(16)))
  bf16 smem[W3_RING * 64 + 2 * W3_PANEL];
  bf16* const ring = smem;                 // [256][64 ci]
  bf16* const ys = smem + W3_RING * 64;    // [2][32][64 co]
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int l16 = lane & 15;
  const int kgrp = lane >> 4;
  const int chunk = blockIdx.x / tiles;
  const int tile = blockIdx.x - chunk * tiles;
  const int to = tile / nt;
  const int co0 = to * 64, ci0 = (tile - to * nt) * 64;
  const int s0 = chunk * spc;
  const int ns = min(spc, steps - s0);
  const long long q0 = (long long)s0 * W3_K;
  const int halo = 2 * g.Wp + 2;

  // staging: thread -> 16-byte chunk (tid & 7) of row (tid >> 3) of a
  // 32-row pass; eight neighbours cover one 128-byte row
  const int srow = tid >> 3, sch = tid & 7;
  const bf16* const px = X + ci0 + sch * 8;
  const bf16* const py = dY + co0 + sch * 8;
  const int ysto = wswz(srow, sch);
  const bf16x8 zv = {(bf16)0.0f, (bf16)0.0f, (bf16)0.0f, (bf16)0.0f,
                     (bf16)0.0f, (bf16)0.0f, (bf16)0.0f, (bf16)0.0f};

  // transposed reads: lane (qq, pp) of a 16-lane group hands in row
  // 8*kgrp + qq (+ 4 for the second read), columns 4pp .. 4pp+3 of a tile
  const int qq = l16 >> 2, pp = l16 & 3;
  const int lrow = 8 * kgrp + qq;
  const int wci = wave * 16;
  const int yo0 = w3_tro(lrow, 0, pp), yo1 = w3_tro(lrow + 4, 0, pp);
  // ring offsets of step 0, per tap and read: the row (below 256) and its
  // swizzle term. A step advances the row by 32, which leaves row & 15 and
  // with it the swizzle term alone: the loop only adds and wraps.
  int xo[9][2];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int hf = 0; hf < 2; ++hf)
      xo[t][hf] =
          w3_tro(lrow + 4 * hf + (t / 3) * g.Wp + (t % 3), wci, pp);

  f32x4 acc[9][4];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[t][j] = (f32x4)0.0f;

  bf16x8 rx, ry;

  // step ks: dY rows q0 + 32ks + srow; the new X rows are ring rows
  // 32ks + halo + srow, virtual pixels q0 + 32ks + srow + W + 3
#define W3_GLOAD(ks)                                                        \
  {                                                                         \
    const long long qy = q0 + (long long)(ks) * W3_K + srow;                \
    const int piy = c3_pixel(qy, g);                                        \
    const int pix = c3_pixel(qy + g.Wp + 1, g);                             \
    ry = piy >= 0 ? *reinterpret_cast<const bf16x8*>(py + (long long)piy * C) \
                  : zv;                                                     \
    rx = pix >= 0 ? *reinterpret_cast<const bf16x8*>(px + (long long)pix * C) \
                  : zv;                                                     \
  }
#define W3_LSTORE(ks)                                                       \
  {                                                                         \
    *reinterpret_cast<bf16x8*>(ys + ((ks) & 1) * W3_PANEL + ysto) = ry;     \
    *reinterpret_cast<bf16x8*>(                                             \
        ring + wswz(((ks) * W3_K + halo + srow) & (W3_RING - 1), sch)) = rx; \
  }

  if (phase_mask & 1) {
    // ring rows [0, 32 + halo): the halo and step 0's new rows
    bf16x8 v[W3_PRO];
#pragma unroll
    for (int u = 0; u < W3_PRO; ++u) {
      const int b = srow + 32 * u;
      const int pix =
          b < W3_K + halo ? c3_pixel(q0 - (g.Wp + 1) + b, g) : -1;
      v[u] = pix >= 0 ? *reinterpret_cast<const bf16x8*>(
                            px + (long long)pix * C)
                      : zv;
    }
    {
      const int piy = c3_pixel(q0 + srow, g);
      ry = piy >= 0 ? *reinterpret_cast<const bf16x8*>(py + (long long)piy * C)
                    : zv;
    }
#pragma unroll
    for (int u = 0; u < W3_PRO; ++u) {
      const int b = srow + 32 * u;
      if (b < W3_K + halo)
        *reinterpret_cast<bf16x8*>(ring + wswz(b, sch)) = v[u];
    }
    *reinterpret_cast<bf16x8*>(ys + ysto) = ry;
  }
  __syncthreads();

#pragma unroll 1
  for (int ks = 0; ks < ns; ++ks) {
    const bool more = ks + 1 < ns;
    if (more && (phase_mask & 1)) W3_GLOAD(ks + 1)
    if (phase_mask & 4) {
      const bf16* yb = ys + (ks & 1) * W3_PANEL;
      bf16x8 yf[4];
#pragma unroll
      for (int j = 0; j < 4; ++j)  // column tile j: chunk index + 2j
        yf[j] = tr_frag(yb + (yo0 ^ (j * 16)), yb + (yo1 ^ (j * 16)));
      const int adv = ks * W3_PANEL;  // 32 ring rows per step
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const bf16x8 xf =
            tr_frag(ring + ((xo[t][0] + adv) & (W3_RING * 64 - 1)),
                    ring + ((xo[t][1] + adv) & (W3_RING * 64 - 1)));
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              xf, yf[j], acc[t][j], 0, 0, 0);
      }
    }
    if (more && (phase_mask & 1)) W3_LSTORE(ks + 1)
    __syncthreads();  // step ks is read, step ks+1 is in place
  }
#undef W3_GLOAD
#undef W3_LSTORE
  if (!(phase_mask & 2)) return;

  // D row = 4*(lane>>4) + r is ci, D col = lane&15 is co: the four
  // registers of a tile are 16 contiguous bytes of part[chunk][co][tap][...]
  float* const my =
      part + ((long long)chunk * C + co0 + l16) * 9 * C + ci0 + wci + 4 * kgrp;
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      *reinterpret_cast<f32x4*>(my + ((long long)j * 16 * 9 + t) * C) =
          acc[t][j];
}

// Chunk count for a request over Q = N(H+2)(W+2) virtual pixels. req > 0
// forces it (clamped to the K-steps); req == 0 takes the smallest count that
// puts about two blocks on every CU of the current device, with chunks of
// at least W3_MIN_STEPS K-steps. Chunks are whole K-steps long and the value
// returned is the effective count ceil(steps / steps_per_chunk): no chunk
// is empty. -1: the device's CU count cannot be read.
extern "C" int conv3x3_wrw_chunks(long long Q, int C, int req) {
  const long long steps = (Q + W3_K - 1) / W3_K;
  long long n = req;
  if (req <= 0) {
    int dev = 0, cus = 0;  // of the current device: callers set it
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                              dev) != hipSuccess || cus <= 0)
      return -1;
    const int tiles = (C / 64) * (C / 64);
    n = (2 * cus + tiles - 1) / tiles;
    if (n > steps / W3_MIN_STEPS) n = steps / W3_MIN_STEPS;
  }
  if (n > steps) n = steps;
  if (n < 1) n = 1;
  const long long spc = (steps + n - 1) / n;
  return (int)((steps + spc - 1) / spc);
}

// x, dy [N,H,W,C]; ``nchunks`` is a value conv3x3_wrw_chunks returned; part
// holds nchunks * 9 * C * C floats, every one of which is written; dw is
// [C,3,3,C] bf16 (a channels-last weight's physical view).
extern "C" void launch_conv3x3_wrw(const void* x, const void* dy, float* part,
                                   void* dw, int N, int H, int W, int C,
                                   int nchunks, int accumulate,
                                   hipStream_t stream, int phase_mask) {
  const C3Geo g = c3_geo(N, H, W);
  const int nt = C / 64, tiles = nt * nt;
  const int steps = (int)(((long long)g.Q + W3_K - 1) / W3_K);
  const int spc = (steps + nchunks - 1) / nchunks;
  hipLaunchKernelGGL(conv3x3_wrw_kernel, dim3((unsigned)nchunks * tiles),
                     dim3(256), 0, stream, (const bf16*)x, (const bf16*)dy,
                     part, C, nt, tiles, spc, steps, phase_mask, g);
  launch_conv_wrw_reduce(part, dw, 9LL * C * C, nchunks, accumulate, stream);
}
