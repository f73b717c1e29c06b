// Fused BatchNorm(+residual)(+ReLU) for gfx950 (MI355X), NHWC bf16.
//
// Replaces the MIOpen spatial-BN path PyTorch-ROCm uses for the ResNet
// family. Profiled on MI355X (profiles/r01_bench_resnet18_1gpu_kernstats.md),
// that path is 4 separate kernels per BN (MeanVariance + Norm forward,
// DScaleDBias + DX backward) run in *fp32* (autocast keeps BN off the
// bf16 list, inserting bfloat16->float32 copy kernels around every BN),
// with the adjacent ReLU and residual-add as further standalone
// elementwise passes — together ~32% of step kernel time.
//
// This file fuses the whole thing at bf16 activation width, with fp32
// accumulation throughout. Each direction is three stream-ordered passes:
//   fwd:  reduce(x) -> finalize -> apply: y = [relu](bn(x) [+ residual])
//   bwd:  reduce(dz, x, mask) -> finalize -> apply: dx [, dres]
//   * reduce: every block sums its rows and writes one slot of a
//     channel-major [2C][nblocks] fp32 partial (block_reduce_store, the
//     one epilogue all five reduce kernels end in). No global atomics:
//     the order of every sum is fixed, so graph replays are bit-stable.
//   * finalize: one wavefront (or block, for long runs) per channel sums
//     the slots. Forward writes mean/invstd, updates the running stats
//     and bumps num_batches_tracked; backward writes dweight/dbias and
//     the three per-channel constants k the apply pass needs.
//   * apply: one streaming pass, one fma-sized expression per element.
// The backward reduce comes in three forms, by where the relu mask and
// the upstream gradient come from:
//   * bn_bwd_reduce: mask from the saved output (y > 0). It can also
//     store the masked gradient dym, which for a residual layer IS the
//     residual branch's gradient and is all the apply pass then reads;
//     and it can sum the gradients of an output's two consumers while it
//     streams (JOIN), so autograd's stand-alone add does not run;
//   * bn_bwd_*_rm (non-residual relu layers): mask recomputed as
//     (w*xhat + b) > 0 from the x already in registers; y is not read;
//   * bn_pool_bwd_* (stem): the same recompute-mask math in the tile
//     order of the 3x3/s2 max-pool, with the un-pooled gradient rebuilt
//     in registers from the pooled gradient and the u8 window codes.
//
// Layout/mapping (CDNA4-first):
//   * activations are NHWC ("channels_last"), rows = N*H*W, C channels
//     contiguous; every load/store is an 8-wide bf16 vector (16 B,
//     dwordx4) so wavefronts of 64 lanes touch 1 KB per instruction.
//   * a block of 256 threads (4 wavefronts) covers 256/(C/8) rows per
//     iteration (RowMap); grid-stride over rows; grids are sized >> 256
//     workgroups where the row count allows, to fill all 8 XCDs.
//   * block-level sums are tree-reduced through LDS (16 KB of the
//     160 KB/CU) before the block's partial slot is written.
// All kernels are stream-ordered device work with no host sync, so
// the whole fused op captures into hipGraphs (train/graphstep.py).
//
// Reference parity: this implements the BatchNorm2d semantics the
// reference's torchvision resnet50 relies on
// (deep_learning/2.distributed-data-loading-petastorm.py:150) including
// running-stat momentum updates and unbiased running variance.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

typedef __hip_bfloat16 bf16;

#define VEC 8  // bf16 elements per vector load/store (16 bytes)

union BVec {
  uint4 u;
  bf16 h[VEC];
};

static __device__ __forceinline__ BVec load8(const bf16* p) {
  BVec v;
  v.u = *reinterpret_cast<const uint4*>(p);
  return v;
}

static __device__ __forceinline__ void store8(bf16* p, const BVec& v) {
  *reinterpret_cast<uint4*>(p) = v.u;
}

// --------------------------------------------------------- shared skeleton
// Thread decomposition of every streaming kernel: `lanes` threads cover
// one row (8 channels each), so a 256-thread block advances
// rows_per_iter rows at a time, grid-stride. The stem's tile-order
// kernels walk 2x2 tiles instead of rows with the same mapping.
//
// Built in two steps, `RowMap t(C); t.span(blockDim.x);`: blockDim.x folds
// to one scalar load only when the __global__ function itself reads it,
// after the lane split (profiles/r07_fused_bn_refactor_isa.md).
struct RowMap {
  int C;
  int lanes;          // vector-lanes per row
  int lane;           // which 8-channel slot
  int rsub;           // row within the block's tile
  int rows_per_iter;
  long long rstride;

  __device__ __forceinline__ explicit RowMap(int C_)
      : C(C_),
        lanes(C_ / VEC),
        lane(threadIdx.x % lanes),
        rsub(threadIdx.x / lanes) {}

  __device__ __forceinline__ void span(unsigned block_threads) {
    rows_per_iter = block_threads / lanes;
    rstride = (long long)gridDim.x * rows_per_iter;
  }

  // this thread's first row (or tile)
  __device__ __forceinline__ long long first_row() const {
    return (long long)blockIdx.x * rows_per_iter + rsub;
  }

  // element offset of this thread's 8 channels in `row`
  __device__ __forceinline__ long long off(long long row) const {
    return row * C + (long long)lane * VEC;
  }
};

// Per-lane channel constants of the backward kernels: mean and invstd, and
// in the second form weight and bias as well (the kernels that recompute
// the relu mask). Loads are issued channel by channel, from per-lane base
// pointers: indexing each vector with lane * VEC + j instead leaves eight
// channel indices live across the kernel's main loop
// (profiles/r07_fused_bn_refactor_isa.md).
static __device__ __forceinline__ void load_stats(
    const RowMap& t, const float* mean, const float* invstd,
    float (&m)[VEC], float (&is)[VEC]) {
  mean += t.lane * VEC;
  invstd += t.lane * VEC;
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    m[j] = mean[j];
    is[j] = invstd[j];
  }
}

static __device__ __forceinline__ void load_stats(
    const RowMap& t, const float* mean, const float* invstd,
    const float* weight, const float* bias, float (&m)[VEC],
    float (&is)[VEC], float (&wv)[VEC], float (&bv)[VEC]) {
  mean += t.lane * VEC;
  invstd += t.lane * VEC;
  weight += t.lane * VEC;
  bias += t.lane * VEC;
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    m[j] = mean[j];
    is[j] = invstd[j];
    wv[j] = weight[j];
    bv[j] = bias[j];
  }
}

// The apply kernels' constants from bn_bwd_finalize: k = [w*invstd,
// mean_dy, mean_dy_xhat], C floats each.
static __device__ __forceinline__ void load_k(
    const RowMap& t, const float* k, float (&wis)[VEC], float (&k1)[VEC],
    float (&k2)[VEC]) {
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    int c = t.lane * VEC + j;
    wis[j] = k[c];
    k1[j] = k[t.C + c];
    k2[j] = k[2 * t.C + c];
  }
}

// Epilogue of every reduce kernel: tree-reduce the block's two per-thread
// accumulators across the rows_per_iter threads sharing each lane, then
// write the block's slot of the channel-major partial [2C][nblocks] (`a`
// to channels [0, C), `b` to [C, 2C)): the finalize wavefront for channel
// c then reads a contiguous nblocks-float run.
//
// Two-stage rather than global atomics — a single fp32 atomic target
// serializes one RMW per block (measured 406 us/call at 2080 blocks on
// MI355X, ~20x the memory-bound cost of the pass) and is
// non-deterministic across graph replays.
static __device__ __forceinline__ void block_reduce_store(
    const RowMap& t, const float (&a)[VEC], const float (&b)[VEC],
    float* partial) {
  __shared__ float lds[256 * 2 * VEC];
  float* mys = &lds[(t.rsub * t.lanes + t.lane) * 2 * VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    mys[j] = a[j];
    mys[VEC + j] = b[j];
  }
  __syncthreads();
  for (int step = t.rows_per_iter >> 1; step > 0; step >>= 1) {
    if (t.rsub < step) {
      const float* other =
          &lds[((t.rsub + step) * t.lanes + t.lane) * 2 * VEC];
#pragma unroll
      for (int j = 0; j < 2 * VEC; ++j) mys[j] += other[j];
    }
    __syncthreads();
  }
  if (t.rsub == 0) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      partial[(long long)(t.lane * VEC + j) * gridDim.x + blockIdx.x] =
          mys[j];
      partial[(long long)(t.C + t.lane * VEC + j) * gridDim.x +
              blockIdx.x] = mys[VEC + j];
    }
  }
}

// ---------------------------------------------------------------- fwd reduce
// partial[c][block] = block-sum x_c, partial[C + c][block] = block-sum
// x_c^2; the finalize kernel sums across blocks.
__global__ __launch_bounds__(256) void bn_fwd_reduce_kernel(
    const bf16* __restrict__ x, float* __restrict__ partial,
    long long rows, int C) {
  RowMap t(C);
  t.span(blockDim.x);
  float s[VEC] = {0.f}, q[VEC] = {0.f};
  for (long long row = t.first_row(); row < rows; row += t.rstride) {
    BVec v = load8(x + t.off(row));
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      float f = __bfloat162float(v.h[j]);
      s[j] += f;
      q[j] += f * f;
    }
  }
  block_reduce_store(t, s, q, partial);
}

// -------------------------------------------------------------- fwd finalize
// Per-channel tail shared by both finalize kernels: statistics out,
// running-stat momentum update, step counter.
static __device__ __forceinline__ void bn_fwd_finalize_channel(
    int c, float s, float q, float* __restrict__ mean,
    float* __restrict__ invstd, float* __restrict__ running_mean,
    float* __restrict__ running_var, float momentum, float eps,
    long long rows, int update_running,
    long long* __restrict__ num_batches_tracked) {
  float n = (float)rows;
  float m = s / n;
  float var = fmaxf(q / n - m * m, 0.f);
  mean[c] = m;
  invstd[c] = rsqrtf(var + eps);
  if (update_running) {
    float unbiased = rows > 1 ? var * (n / (n - 1.f)) : var;
    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * m;
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * unbiased;
  }
  if (c == 0 && num_batches_tracked) *num_batches_tracked += 1;
}

// One 64-lane wavefront per channel: lanes stride the [nblocks] partial
// run (coalesced), then an in-wavefront shuffle tree. mean/invstd out +
// momentum update of running stats (unbiased running var, matching torch
// BatchNorm2d). Device-side so it replays inside hipGraphs; fixed
// summation order = deterministic. When num_batches_tracked is non-null
// the channel-0 lane-0 thread also bumps the module's int64 step counter,
// so the training forward needs no separate `+= 1` elementwise kernel.
__global__ __launch_bounds__(256) void bn_fwd_finalize_kernel(
    const float* __restrict__ partial, int nblocks,
    float* __restrict__ mean, float* __restrict__ invstd,
    float* __restrict__ running_mean, float* __restrict__ running_var,
    float momentum, float eps, long long rows, int C, int update_running,
    long long* __restrict__ num_batches_tracked) {
  int c = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
  int lane = threadIdx.x % 64;
  if (c >= C) return;
  float s = 0.f, q = 0.f;
  for (int b = lane; b < nblocks; b += 64) {
    s += partial[(long long)c * nblocks + b];
    q += partial[(long long)(C + c) * nblocks + b];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s += __shfl_down(s, off, 64);
    q += __shfl_down(q, off, 64);
  }
  if (lane != 0) return;
  bn_fwd_finalize_channel(c, s, q, mean, invstd, running_mean, running_var,
                          momentum, eps, rows, update_running,
                          num_batches_tracked);
}

// Same result layout, for LONG partial runs: one 256-thread block per
// channel instead of one wavefront. The stem conv's epilogue leaves one
// slot per block of its own grid (2,968 at the flagship shape against the
// reduce kernels' <= 512): a single wavefront then walks 46 dependent
// iterations per channel (measured 19.3 us against 9.7 us at 512 slots).
// Lanes stride the run with four independent loads in flight, then
// shuffle tree per wavefront and a fixed-order sum of the four wavefront
// totals: deterministic.
__global__ __launch_bounds__(256) void bn_fwd_finalize_wide_kernel(
    const float* __restrict__ partial, int nblocks,
    float* __restrict__ mean, float* __restrict__ invstd,
    float* __restrict__ running_mean, float* __restrict__ running_var,
    float momentum, float eps, long long rows, int C, int update_running,
    long long* __restrict__ num_batches_tracked) {
  const int c = blockIdx.x;
  const int tid = threadIdx.x;
  const float* ps = partial + (long long)c * nblocks;
  const float* pq = partial + (long long)(C + c) * nblocks;
  float s4[4] = {0.f, 0.f, 0.f, 0.f}, q4[4] = {0.f, 0.f, 0.f, 0.f};
  int b = tid;
  for (; b + 3 * 256 < nblocks; b += 4 * 256) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      s4[u] += ps[b + u * 256];
      q4[u] += pq[b + u * 256];
    }
  }
  for (; b < nblocks; b += 256) {
    s4[0] += ps[b];
    q4[0] += pq[b];
  }
  float s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
  float q = (q4[0] + q4[1]) + (q4[2] + q4[3]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s += __shfl_down(s, off, 64);
    q += __shfl_down(q, off, 64);
  }
  __shared__ float ws[4], wq[4];
  if ((tid & 63) == 0) {
    ws[tid >> 6] = s;
    wq[tid >> 6] = q;
  }
  __syncthreads();
  if (tid != 0) return;
  s = (ws[0] + ws[1]) + (ws[2] + ws[3]);
  q = (wq[0] + wq[1]) + (wq[2] + wq[3]);
  bn_fwd_finalize_channel(c, s, q, mean, invstd, running_mean, running_var,
                          momentum, eps, rows, update_running,
                          num_batches_tracked);
}

// ---------------------------------------------------------------- fwd apply
// y = relu?( (x - mean)*invstd*w + b  (+ residual) ), all bf16 I/O.
// Per-thread channel constants are folded once: a = w*invstd,
// b' = b - mean*a, so the inner loop is one fma per element.
template <bool RELU, bool RES>
__global__ __launch_bounds__(256) void bn_fwd_apply_kernel(
    const bf16* __restrict__ x, const bf16* __restrict__ res,
    bf16* __restrict__ y, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ weight,
    const float* __restrict__ bias, long long rows, int C) {
  RowMap t(C);
  t.span(blockDim.x);
  float a[VEC], b[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    int c = t.lane * VEC + j;
    a[j] = weight[c] * invstd[c];
    b[j] = bias[c] - mean[c] * a[j];
  }

  for (long long row = t.first_row(); row < rows; row += t.rstride) {
    const long long off = t.off(row);
    BVec v = load8(x + off);
    BVec r;
    if (RES) r = load8(res + off);
    BVec o;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      float f = fmaf(__bfloat162float(v.h[j]), a[j], b[j]);
      if (RES) f += __bfloat162float(r.h[j]);
      if (RELU) f = fmaxf(f, 0.f);
      o.h[j] = __float2bfloat16(f);
    }
    store8(y + off, o);
  }
}

// ---------------------------------------------------------------- bwd reduce
// dy = relu-masked upstream grad (mask = saved y > 0); partial holds the
// block sums of dy and dy*xhat. When WRITE_DY, the masked dy is also
// materialized to dym: for residual layers dym IS the residual-branch
// gradient, and the apply pass then reads (dym, x) instead of (dz, y, x)
// — one read and one write less per layer.
//
// JOIN is the residual-layer reduce for an output with TWO consumers (the
// next block's conv1 and its identity path / downsample conv). Autograd
// would sum the two incoming gradients with a stand-alone elementwise add
// (2 maps read, 1 written) right in front of this kernel, which reads
// that sum exactly once. Here the kernel reads both addends itself: one
// extra map read, no add kernel. Per element dy = bf16(float(dz) +
// float(dz2)), widened again — exactly the value the bf16 add kernel
// stored — so mask, sdy, sdyx and dym are bit-identical to the one-gradient
// kernel run on the summed map. All four 16 B loads of a row are issued
// before the first use.
template <bool RELU, bool WRITE_DY, bool JOIN>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(
    const bf16* __restrict__ dz, const bf16* __restrict__ dz2,
    const bf16* __restrict__ y, const bf16* __restrict__ x,
    const float* __restrict__ mean, const float* __restrict__ invstd,
    float* __restrict__ partial, bf16* __restrict__ dym, long long rows,
    int C) {
  RowMap t(C);
  t.span(blockDim.x);
  float m[VEC], is[VEC];
  load_stats(t, mean, invstd, m, is);

  float sdy[VEC] = {0.f}, sdyx[VEC] = {0.f};
  for (long long row = t.first_row(); row < rows; row += t.rstride) {
    const long long off = t.off(row);
    BVec g = load8(dz + off);
    BVec g2;
    if (JOIN) g2 = load8(dz2 + off);
    BVec xv = load8(x + off);
    BVec yv;
    if (RELU) yv = load8(y + off);
    BVec dyv;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      float dy = __bfloat162float(g.h[j]);
      // round the sum to bf16 first: that is what the add kernel stored
      if (JOIN)
        dy = __bfloat162float(
            __float2bfloat16(dy + __bfloat162float(g2.h[j])));
      if (RELU && __bfloat162float(yv.h[j]) <= 0.f) dy = 0.f;
      float xhat = (__bfloat162float(xv.h[j]) - m[j]) * is[j];
      sdy[j] += dy;
      sdyx[j] += dy * xhat;
      if (WRITE_DY) dyv.h[j] = __float2bfloat16(dy);
    }
    if (WRITE_DY) store8(dym + off, dyv);
  }
  block_reduce_store(t, sdy, sdyx, partial);
}

// -------------------------------------------------------------- bwd finalize
// One 64-lane wavefront per channel (same scheme as forward finalize):
// dweight = sum dy*xhat ; dbias = sum dy ; k = [w*invstd, mean_dy,
// mean_dy_xhat] per channel for the apply pass.
__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(
    const float* __restrict__ partial, int nblocks,
    const float* __restrict__ invstd, const float* __restrict__ weight,
    float* __restrict__ dweight, float* __restrict__ dbias,
    float* __restrict__ k, long long rows, int C, int accumulate) {
  int c = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
  int lane = threadIdx.x % 64;
  if (c >= C) return;
  float sdy = 0.f, sdyx = 0.f;
  for (int b = lane; b < nblocks; b += 64) {
    sdy += partial[(long long)c * nblocks + b];
    sdyx += partial[(long long)(C + c) * nblocks + b];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    sdy += __shfl_down(sdy, off, 64);
    sdyx += __shfl_down(sdyx, off, 64);
  }
  if (lane != 0) return;
  // accumulate=1: write straight into the flat grad views (graph-capture
  // path) so autograd's per-param AccumulateGrad add kernels disappear
  dbias[c] = accumulate ? dbias[c] + sdy : sdy;
  dweight[c] = accumulate ? dweight[c] + sdyx : sdyx;
  k[c] = weight[c] * invstd[c];  // the dx scale factor
  k[C + c] = sdy / (float)rows;
  k[2 * C + c] = sdyx / (float)rows;
}

// ---------------------------------------------------------------- bwd apply
// dx = w*invstd * (dy - mean_dy - xhat*mean_dy_xhat), with xhat
// recomputed from (x-mean)*invstd and dy relu-masked; dres = dy.
// <false, false> is also the residual layers' second pass: given the
// pre-masked dym the reduce wrote as dz, it reads (dym, x) and never y.
template <bool RELU, bool RES>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(
    const bf16* __restrict__ dz, const bf16* __restrict__ y,
    const bf16* __restrict__ x, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ k,
    bf16* __restrict__ dx, bf16* __restrict__ dres, long long rows, int C) {
  RowMap t(C);
  t.span(blockDim.x);
  float m[VEC], is[VEC], wis[VEC], k1[VEC], k2[VEC];
  load_stats(t, mean, invstd, m, is);
  load_k(t, k, wis, k1, k2);

  for (long long row = t.first_row(); row < rows; row += t.rstride) {
    const long long off = t.off(row);
    BVec g = load8(dz + off);
    BVec xv = load8(x + off);
    BVec yv;
    if (RELU) yv = load8(y + off);
    BVec odx, odr;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      float dy = __bfloat162float(g.h[j]);
      if (RELU && __bfloat162float(yv.h[j]) <= 0.f) dy = 0.f;
      float xhat = (__bfloat162float(xv.h[j]) - m[j]) * is[j];
      float v = wis[j] * (dy - k1[j] - xhat * k2[j]);
      odx.h[j] = __float2bfloat16(v);
      if (RES) odr.h[j] = __float2bfloat16(dy);
    }
    store8(dx + off, odx);
    if (RES) store8(dres + off, odr);
  }
}

// ---------------------------------------------------- recompute-mask bwd
// Non-residual RELU backward: the stored y is read ONLY for the relu
// mask, which is recomputable as (w*xhat + b) > 0 from the x already in
// registers — one full activation-map read drops out of BOTH backward
// passes (and y need not be saved for backward at all). The fp32
// recompute is if anything closer to the fp32 reference than masking on
// the rounded bf16 y. Residual layers keep the y path (the mask there
// depends on the residual input).
//
// The per-element arithmetic of the recompute-mask path lives in the three
// helpers below, with its fused multiply-adds spelled out. The row-order
// rm kernels and the stem's tile-order bn_pool_bwd_* kernels all call
// them, so the two paths round identically by construction, whatever the
// compiler's contraction choices are for either loop shape.
static __device__ __forceinline__ float rm_masked_dy(float dy, float w,
                                                     float xhat, float b) {
  if (fmaf(w, xhat, b) <= 0.f) dy = 0.f;
  return dy;
}

static __device__ __forceinline__ void rm_accumulate(float dy, float xhat,
                                                     float& sdy,
                                                     float& sdyx) {
  sdy += dy;
  sdyx = fmaf(dy, xhat, sdyx);
}

// dx = w*invstd * (dy - mean_dy - xhat*mean_dy_xhat)
static __device__ __forceinline__ float rm_dx(float wis, float dy, float k1,
                                              float xhat, float k2) {
  return wis * fmaf(-xhat, k2, dy - k1);
}

template <bool WRITE_DY>
__global__ __launch_bounds__(256) void bn_bwd_reduce_rm_kernel(
    const bf16* __restrict__ dz, const bf16* __restrict__ x,
    const float* __restrict__ mean, const float* __restrict__ invstd,
    const float* __restrict__ weight, const float* __restrict__ bias,
    float* __restrict__ partial, bf16* __restrict__ dym,
    long long rows, int C) {
  RowMap t(C);
  t.span(blockDim.x);
  float m[VEC], is[VEC], wv[VEC], bv[VEC];
  load_stats(t, mean, invstd, weight, bias, m, is, wv, bv);

  float sdy[VEC] = {0.f}, sdyx[VEC] = {0.f};
  for (long long row = t.first_row(); row < rows; row += t.rstride) {
    const long long off = t.off(row);
    BVec g = load8(dz + off);
    BVec xv = load8(x + off);
    BVec dyv;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      float xhat = (__bfloat162float(xv.h[j]) - m[j]) * is[j];
      float dy = rm_masked_dy(__bfloat162float(g.h[j]), wv[j], xhat, bv[j]);
      rm_accumulate(dy, xhat, sdy[j], sdyx[j]);
      if (WRITE_DY) dyv.h[j] = __float2bfloat16(dy);
    }
    if (WRITE_DY) store8(dym + off, dyv);
  }
  block_reduce_store(t, sdy, sdyx, partial);
}

__global__ __launch_bounds__(256) void bn_bwd_apply_rm_kernel(
    const bf16* __restrict__ dz, const bf16* __restrict__ x,
    const float* __restrict__ mean, const float* __restrict__ invstd,
    const float* __restrict__ bias, const float* __restrict__ k,
    bf16* __restrict__ dx, long long rows, int C) {
  RowMap t(C);
  t.span(blockDim.x);
  float m[VEC], is[VEC], wis[VEC], k1[VEC], k2[VEC], bv[VEC], wv[VEC];
  load_stats(t, mean, invstd, m, is);
  load_k(t, k, wis, k1, k2);
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    bv[j] = bias[t.lane * VEC + j];
    wv[j] = wis[j] / is[j];  // w, recovered once per channel
  }

  for (long long row = t.first_row(); row < rows; row += t.rstride) {
    const long long off = t.off(row);
    BVec g = load8(dz + off);
    BVec xv = load8(x + off);
    BVec odx;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      float xhat = (__bfloat162float(xv.h[j]) - m[j]) * is[j];
      float dy = rm_masked_dy(__bfloat162float(g.h[j]), wv[j], xhat, bv[j]);
      float v = rm_dx(wis[j], dy, k1[j], xhat, k2[j]);
      odx.h[j] = __float2bfloat16(v);
    }
    store8(dx + off, odx);
  }
}

// ------------------------------------------------- stem bwd, un-pool fused
// The stem's backward used to run maxpool3x3s2_bwd -> reduce_rm -> apply_rm:
// the un-pooled gradient map dz (same size as x, 340 MB at bs 212) was
// written once and read twice, although it is only a sparse scatter of
// the pooled grad dp selected by the u8 window code. The two kernels
// below rebuild the tile's four dz values in registers instead, so dz is
// never materialized.
//
// Mapping is maxpool_bwd_kernel's (maxpool.hip): one thread-lane owns the
// 2x2 input tile at (2i, 2j) for 8 channels; tiles == the pooled grid.
// Each of the tile's pixels sits at a fixed position inside the (up to)
// four windows that touch it, so every dp/code vector is loaded once and
// all code compares are against constants. Each un-pooled value is
// rounded to bf16 and widened again so it equals what maxpool_bwd_kernel
// would have stored. (The tile code is repeated here rather than shared
// through a header: a local header makes the extension build emit
// hipified copies of both .hip files into the source tree.)
union CVec {
  uint2 u;
  unsigned char c[VEC];
};

// Tile decomposition shared by both passes. pix[p] is the NHWC element
// offset of tile pixel p (0:(2i,2j) 1:(2i,2j+1) 2:(2i+1,2j) 3:(2i+1,2j+1)),
// valid[p] its in-image guard for odd H / W.
struct PoolTile {
  float a[4][VEC];
  long long pix[4];
  bool valid[4];
};

static __device__ __forceinline__ void unpool_tile(
    const bf16* __restrict__ dp, const unsigned char* __restrict__ code,
    int r32, int lane, int H, int W, int Ho, int Wo, int C, PoolTile& t) {
  const int j = r32 % Wo;
  const int t32 = r32 / Wo;
  const int i = t32 % Ho;
  const int n = t32 / Ho;
  const long long lvec = (long long)lane * VEC;

  BVec g00{}, g01{}, g10{}, g11{};
  CVec c00{}, c01{}, c10{}, c11{};
  const bool v01 = (j + 1 < Wo), v10 = (i + 1 < Ho);
  const long long base = (((long long)n * Ho + i) * Wo + j) * C + lvec;
  g00.u = *reinterpret_cast<const uint4*>(dp + base);
  c00.u = *reinterpret_cast<const uint2*>(code + base);
  if (v01) {
    g01.u = *reinterpret_cast<const uint4*>(dp + base + C);
    c01.u = *reinterpret_cast<const uint2*>(code + base + C);
  }
  if (v10) {
    const long long b2 = base + (long long)Wo * C;
    g10.u = *reinterpret_cast<const uint4*>(dp + b2);
    c10.u = *reinterpret_cast<const uint2*>(code + b2);
    if (v01) {
      g11.u = *reinterpret_cast<const uint4*>(dp + b2 + C);
      c11.u = *reinterpret_cast<const uint2*>(code + b2 + C);
    }
  }
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    float a00 = (c00.c[k] == 4) ? __bfloat162float(g00.h[k]) : 0.f;
    float a01 = (c00.c[k] == 5) ? __bfloat162float(g00.h[k]) : 0.f;
    if (v01 && c01.c[k] == 3) a01 += __bfloat162float(g01.h[k]);
    float a10 = (c00.c[k] == 7) ? __bfloat162float(g00.h[k]) : 0.f;
    if (v10 && c10.c[k] == 1) a10 += __bfloat162float(g10.h[k]);
    float a11 = (c00.c[k] == 8) ? __bfloat162float(g00.h[k]) : 0.f;
    if (v01 && c01.c[k] == 6) a11 += __bfloat162float(g01.h[k]);
    if (v10 && c10.c[k] == 2) a11 += __bfloat162float(g10.h[k]);
    if (v10 && v01 && c11.c[k] == 0) a11 += __bfloat162float(g11.h[k]);
    t.a[0][k] = __bfloat162float(__float2bfloat16(a00));
    t.a[1][k] = __bfloat162float(__float2bfloat16(a01));
    t.a[2][k] = __bfloat162float(__float2bfloat16(a10));
    t.a[3][k] = __bfloat162float(__float2bfloat16(a11));
  }
  const int h0 = 2 * i, w0 = 2 * j;
  const bool r1 = (h0 + 1 < H), cL1 = (w0 + 1 < W);
  const long long ibase = (((long long)n * H + h0) * W + w0) * C + lvec;
  t.pix[0] = ibase;
  t.pix[1] = ibase + C;
  t.pix[2] = ibase + (long long)W * C;
  t.pix[3] = ibase + (long long)W * C + C;
  t.valid[0] = true;
  t.valid[1] = cL1;
  t.valid[2] = r1;
  t.valid[3] = r1 && cL1;
}

// Same math, LDS tree and [2C][nblocks] partial layout as
// bn_bwd_reduce_rm_kernel<false>, so bn_bwd_finalize is reused unchanged;
// only the fp32 summation order differs (tile order, not row order).
//
// Per-element math goes through the rm_* helpers shared with the rm
// kernels (explicit fmaf): here the per-pixel edge guards split the loop
// body into basic blocks, and left to the compiler, contraction would not
// cross them and some pixels would round differently from the unfused
// path.
__global__ __launch_bounds__(256) void bn_pool_bwd_reduce_kernel(
    const bf16* __restrict__ dp, const unsigned char* __restrict__ code,
    const bf16* __restrict__ x, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ weight,
    const float* __restrict__ bias, float* __restrict__ partial, int N,
    int H, int W, int Ho, int Wo, int C) {
  const long long tiles = (long long)N * Ho * Wo;
  RowMap t(C);
  t.span(blockDim.x);
  float m[VEC], is[VEC], wv[VEC], bv[VEC];
  load_stats(t, mean, invstd, weight, bias, m, is, wv, bv);

  float sdy[VEC] = {0.f}, sdyx[VEC] = {0.f};
  for (long long tile = t.first_row(); tile < tiles; tile += t.rstride) {
    PoolTile pt;
    unpool_tile(dp, code, (int)tile, t.lane, H, W, Ho, Wo, C, pt);
    BVec xv[4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
      if (pt.valid[p]) xv[p] = load8(x + pt.pix[p]);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      if (!pt.valid[p]) continue;
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        float xhat = (__bfloat162float(xv[p].h[j]) - m[j]) * is[j];
        float dy = rm_masked_dy(pt.a[p][j], wv[j], xhat, bv[j]);
        rm_accumulate(dy, xhat, sdy[j], sdyx[j]);
      }
    }
  }
  block_reduce_store(t, sdy, sdyx, partial);
}

// Arithmetic is bn_bwd_apply_rm_kernel's (the shared rm_* helpers, and
// wv = wis / is), so given the same k the dx map is bit-identical to the
// unfused path.
__global__ __launch_bounds__(256) void bn_pool_bwd_apply_kernel(
    const bf16* __restrict__ dp, const unsigned char* __restrict__ code,
    const bf16* __restrict__ x, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ bias,
    const float* __restrict__ k, bf16* __restrict__ dx, int N, int H, int W,
    int Ho, int Wo, int C) {
  const long long tiles = (long long)N * Ho * Wo;
  RowMap t(C);
  t.span(blockDim.x);
  float m[VEC], is[VEC], wis[VEC], k1[VEC], k2[VEC], bv[VEC], wv[VEC];
  load_stats(t, mean, invstd, m, is);
  load_k(t, k, wis, k1, k2);
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    bv[j] = bias[t.lane * VEC + j];
    wv[j] = wis[j] / is[j];  // w, recovered once per channel
  }

  for (long long tile = t.first_row(); tile < tiles; tile += t.rstride) {
    PoolTile pt;
    unpool_tile(dp, code, (int)tile, t.lane, H, W, Ho, Wo, C, pt);
    BVec xv[4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
      if (pt.valid[p]) xv[p] = load8(x + pt.pix[p]);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      if (!pt.valid[p]) continue;
      BVec odx;
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        float xhat = (__bfloat162float(xv[p].h[j]) - m[j]) * is[j];
        float dy = rm_masked_dy(pt.a[p][j], wv[j], xhat, bv[j]);
        float v = rm_dx(wis[j], dy, k1[j], xhat, k2[j]);
        odx.h[j] = __float2bfloat16(v);
      }
      store8(dx + pt.pix[p], odx);
    }
  }
}

// ------------------------------------------------------------------ launchers

// One block advances 256/(C/8) rows per iteration; enough blocks to cover
// the rows once, up to `cap`, so small late-layer maps don't launch empty
// blocks.
static int grid_blocks(long long rows, int C, long long cap) {
  int rows_per_iter = 256 / (C / VEC);
  long long blocks = (rows + rows_per_iter - 1) / rows_per_iter;
  if (blocks > cap) blocks = cap;
  return (int)(blocks > 0 ? blocks : 1);
}

static int pick_grid(long long rows, int C) {
  return grid_blocks(rows, C, 2080);  // 8.1 per CU; multiple of 8 XCDs + 1
}

// Reduce grids are capped lower: 512 blocks (2/CU) saturate HBM on a
// pure-read pass and bound the partial buffer at 512*2C floats.
extern "C" int bn_reduce_blocks(long long rows, int C) {
  return grid_blocks(rows, C, 512);
}

extern "C" void launch_bn_fwd_reduce(const void* x, float* partial,
                                     int nblocks, long long rows, int C,
                                     hipStream_t stream) {
  hipLaunchKernelGGL(bn_fwd_reduce_kernel, dim3(nblocks), dim3(256), 0,
                     stream, (const bf16*)x, partial, rows, C);
}

// Above this many partial slots per channel the block-per-channel
// finalize runs. Every reduce kernel of this file stays below it
// (bn_reduce_blocks caps at 512), so their results are untouched.
#define BN_FINALIZE_WIDE_MIN 1024

extern "C" void launch_bn_fwd_finalize(const float* partial, int nblocks,
                                       float* mean, float* invstd,
                                       float* running_mean,
                                       float* running_var, float momentum,
                                       float eps, long long rows, int C,
                                       int update_running,
                                       long long* num_batches_tracked,
                                       hipStream_t stream) {
  if (nblocks > BN_FINALIZE_WIDE_MIN) {  // long runs: a block per channel
    hipLaunchKernelGGL(bn_fwd_finalize_wide_kernel, dim3(C), dim3(256), 0,
                       stream, partial, nblocks, mean, invstd, running_mean,
                       running_var, momentum, eps, rows, C, update_running,
                       num_batches_tracked);
    return;
  }
  // 4 wavefronts (= 4 channels) per block
  hipLaunchKernelGGL(bn_fwd_finalize_kernel, dim3((C + 3) / 4),
                     dim3(256), 0, stream, partial, nblocks, mean, invstd,
                     running_mean, running_var, momentum, eps, rows, C,
                     update_running, num_batches_tracked);
}

extern "C" void launch_bn_fwd_apply(const void* x, const void* res, void* y,
                                    const float* mean, const float* invstd,
                                    const float* weight, const float* bias,
                                    long long rows, int C, int relu,
                                    hipStream_t stream) {
  dim3 grid(pick_grid(rows, C)), block(256);
#define APPLY(R, S)                                                       \
  hipLaunchKernelGGL((bn_fwd_apply_kernel<R, S>), grid, block, 0, stream, \
                     (const bf16*)x, (const bf16*)res, (bf16*)y, mean,    \
                     invstd, weight, bias, rows, C)
  if (relu && res) APPLY(true, true);
  else if (relu) APPLY(true, false);
  else if (res) APPLY(false, true);
  else APPLY(false, false);
#undef APPLY
}

// dz2 non-null selects the joined form (dz + dz2 summed in the kernel),
// which always writes dym.
extern "C" void launch_bn_bwd_reduce(const void* dz, const void* dz2,
                                     const void* y, const void* x,
                                     const float* mean, const float* invstd,
                                     float* partial, void* dym, int nblocks,
                                     long long rows, int C, int relu,
                                     hipStream_t stream) {
  dim3 grid(nblocks), block(256);
#define REDUCE(R, W, J)                                                   \
  hipLaunchKernelGGL((bn_bwd_reduce_kernel<R, W, J>), grid, block, 0,     \
                     stream, (const bf16*)dz, (const bf16*)dz2,           \
                     (const bf16*)y, (const bf16*)x, mean, invstd,        \
                     partial, (bf16*)dym, rows, C)
  if (dz2 && relu) REDUCE(true, true, true);
  else if (dz2) REDUCE(false, true, true);
  else if (relu && dym) REDUCE(true, true, false);
  else if (relu) REDUCE(true, false, false);
  else if (dym) REDUCE(false, true, false);
  else REDUCE(false, false, false);
#undef REDUCE
}

extern "C" void launch_bn_bwd_reduce_rm(const void* dz, const void* x,
                                        const float* mean,
                                        const float* invstd,
                                        const float* weight,
                                        const float* bias, float* partial,
                                        void* dym, int nblocks,
                                        long long rows, int C,
                                        hipStream_t stream) {
  dim3 grid(nblocks), block(256);
  if (dym)
    hipLaunchKernelGGL((bn_bwd_reduce_rm_kernel<true>), grid, block, 0,
                       stream, (const bf16*)dz, (const bf16*)x, mean,
                       invstd, weight, bias, partial, (bf16*)dym, rows, C);
  else
    hipLaunchKernelGGL((bn_bwd_reduce_rm_kernel<false>), grid, block, 0,
                       stream, (const bf16*)dz, (const bf16*)x, mean,
                       invstd, weight, bias, partial, nullptr, rows, C);
}

extern "C" void launch_bn_bwd_apply_rm(const void* dz, const void* x,
                                       const float* mean,
                                       const float* invstd,
                                       const float* bias, const float* k,
                                       void* dx, long long rows, int C,
                                       hipStream_t stream) {
  hipLaunchKernelGGL(bn_bwd_apply_rm_kernel, dim3(pick_grid(rows, C)),
                     dim3(256), 0, stream, (const bf16*)dz,
                     (const bf16*)x, mean, invstd, bias, k, (bf16*)dx,
                     rows, C);
}

// Stem pair: the grids are sized over the tile count N*Ho*Wo (the caller
// passes nblocks = bn_reduce_blocks(tiles, C) for the reduce).
extern "C" void launch_bn_pool_bwd_reduce(
    const void* dp, const unsigned char* code, const void* x,
    const float* mean, const float* invstd, const float* weight,
    const float* bias, float* partial, int nblocks, int N, int H, int W,
    int Ho, int Wo, int C, hipStream_t stream) {
  hipLaunchKernelGGL(bn_pool_bwd_reduce_kernel, dim3(nblocks), dim3(256), 0,
                     stream, (const bf16*)dp, code, (const bf16*)x, mean,
                     invstd, weight, bias, partial, N, H, W, Ho, Wo, C);
}

extern "C" void launch_bn_pool_bwd_apply(
    const void* dp, const unsigned char* code, const void* x,
    const float* mean, const float* invstd, const float* bias,
    const float* k, void* dx, int N, int H, int W, int Ho, int Wo, int C,
    hipStream_t stream) {
  hipLaunchKernelGGL(bn_pool_bwd_apply_kernel,
                     dim3(pick_grid((long long)N * Ho * Wo, C)), dim3(256),
                     0, stream, (const bf16*)dp, code, (const bf16*)x, mean,
                     invstd, bias, k, (bf16*)dx, N, H, W, Ho, Wo, C);
}

extern "C" void launch_bn_bwd_finalize(const float* partial, int nblocks,
                                       const float* invstd,
                                       const float* weight, float* dweight,
                                       float* dbias, float* k, long long rows,
                                       int C, int accumulate,
                                       hipStream_t stream) {
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((C + 3) / 4),
                     dim3(256), 0, stream, partial, nblocks, invstd, weight,
                     dweight, dbias, k, rows, C, accumulate);
}

extern "C" void launch_bn_bwd_apply(const void* dz, const void* y,
                                    const void* x, const float* mean,
                                    const float* invstd, const float* k,
                                    void* dx, void* dres, long long rows,
                                    int C, int relu, hipStream_t stream) {
  dim3 grid(pick_grid(rows, C)), block(256);
#define APPLY(R, S)                                                        \
  hipLaunchKernelGGL((bn_bwd_apply_kernel<R, S>), grid, block, 0, stream,  \
                     (const bf16*)dz, (const bf16*)y, (const bf16*)x,      \
                     mean, invstd, k, (bf16*)dx, (bf16*)dres, rows, C)
  if (relu && dres) APPLY(true, true);
  else if (relu) APPLY(true, false);
  else if (dres) APPLY(false, true);
  else APPLY(false, false);
#undef APPLY
}

// Residual layers' second pass: dym is already masked and doubles as the
// residual gradient, so this is the plain apply with no y and no dres.
extern "C" void launch_bn_bwd_apply_dym(const void* dym, const void* x,
                                        const float* mean,
                                        const float* invstd, const float* k,
                                        void* dx, long long rows, int C,
                                        hipStream_t stream) {
  launch_bn_bwd_apply(dym, nullptr, x, mean, invstd, k, dx, nullptr, rows, C,
                      0, stream);
}
