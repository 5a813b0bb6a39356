// The rec step of the inner-product recommenders (FM fm.py:58-67, coFM cofm.py:99-108, CKE CKE.py:122-135; BPRMF without the
// options) in ONE launch, and the alignment term of the joint baselines (knowledgable_recommendation.py:385-390) -- see
// include/ktup_hip.h.
//
// dot_step_kernel: a gather and scatter of at most five rows per example; latency and atomic traffic bound it, not arithmetic.
// One wave64 owns an example (four examples in flight per workgroup): it reads the user row and the positive and negative
// item-side rows ONCE for both directions, reduces the two dots across its lanes, evaluates the BPR term and its derivative on every
// lane (no broadcast needed after the xor-shuffle reduction) and adds the three to five gradient rows with float atomics -- the user
// row once per example, because a user is shared by its positive and its negative pair.  The workgroup's loss partial leaves with
// one atomic.  Up to 4 columns per lane (float4: d <= 256 is one chunk per lane; element-wise: up to four) cover d <= 256.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ktup_rows.h"

using namespace ktup;

namespace {

constexpr int MAX_D = 256;

// -log(sigmoid(x)) the way torch's logsigmoid evaluates it (ktup_loss.hip pair_loss_fused_kernel)
KTUP_DEV float neg_logsigmoid(float x) { return fmaxf(-x, 0.f) + log1pf(expf(-fabsf(x))); }
KTUP_DEV float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

// Sum of one float per wave over the workgroup's four waves; valid in thread 0.
KTUP_DEV float block_sum_waves(float wave_total, float* red) {
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = wave_total;
  __syncthreads();
  return threadIdx.x == 0 ? (red[0] + red[1]) + (red[2] + red[3]) : 0.f;
}

struct DotStepArgs {
  const float *U, *I, *X;
  int64_t ldu, ldi, ldx;
  const int64_t* xmap;
  int64_t x_pad;
  const float *gbias, *bu, *bi;
  const int64_t *u_ids, *i_ids;
  int64_t B;
  float target, up;
  float* loss;
  float *gU, *gI, *gX, *gbi;
  int nch;  // chunks of V per row
};

template <typename V, int CPL>
__global__ __launch_bounds__(256) void dot_step_kernel(DotStepArgs a) {
  __shared__ float red[4];
  const RowCtx<V, 64, CPL> cx{a.nch, (int)(threadIdx.x & 63)};
  const float gb = a.gbias ? a.gbias[0] : 0.f;
  const float gmean = a.up / (float)a.B;
  float part = 0.f;
  for (int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); k < a.B; k += (int64_t)gridDim.x * 4) {
    const int64_t u = a.u_ids[k], ip = a.i_ids[k], in = a.i_ids[a.B + k];
    V ur[CPL], vp[CPL], vn[CPL];
    cx.load(ur, a.U + u * a.ldu);
    cx.load(vp, a.I + ip * a.ldi);
    cx.load(vn, a.I + in * a.ldi);
    int64_t xp = 0, xn = 0;
    if (a.X) {
      xp = a.xmap[ip];
      xn = a.xmap[in];
      V ep[CPL], en[CPL];
      cx.load(ep, a.X + xp * a.ldx);
      cx.load(en, a.X + xn * a.ldx);
#pragma unroll
      for (int j = 0; j < CPL; ++j) { vp[j] = vadd(vp[j], ep[j]); vn[j] = vadd(vn[j], en[j]); }
    }
    float dp = 0.f, dn = 0.f;
#pragma unroll
    for (int j = 0; j < CPL; ++j) { dp += vdot(ur[j], vp[j]); dn += vdot(ur[j], vn[j]); }
    dp = group_sum<64>(dp);
    dn = group_sum<64>(dn);
    // ((gbias + bu[u]) + bi[i]) + dot: the additions of fm.py:45 in their order, absent terms skipped
    float sp = dp, sn = dn;
    if (a.gbias || a.bu || a.bi) {
      float hp = 0.f, hn = 0.f;
      bool have = false;
      if (a.gbias) { hp = hn = gb; have = true; }
      if (a.bu) { const float b = a.bu[u]; hp = have ? hp + b : b; hn = hp; have = true; }
      if (a.bi) { const float bp = a.bi[ip], bn = a.bi[in]; hp = have ? hp + bp : bp; hn = have ? hn + bn : bn; }
      sp = hp + dp;
      sn = hn + dn;
    }
    const float x = a.target * (sp - sn);
    part += neg_logsigmoid(x);                                      // (the same value on every lane; lane 0's is used)
    const float g = -gmean * a.target * sigmoidf(-x);               // d/d s_pos; -g is d/d s_neg
    V gu[CPL], gi[CPL], gn[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      gu[j] = vscale(g, vsub(vp[j], vn[j]));
      gi[j] = vscale(g, ur[j]);
      gn[j] = vscale(-g, ur[j]);
    }
    cx.scatter_add(a.gU + u * a.ldu, gu);
    cx.scatter_add(a.gI + ip * a.ldi, gi);
    cx.scatter_add(a.gI + in * a.ldi, gn);
    if (a.X) {
      if (xp != a.x_pad) cx.scatter_add(a.gX + xp * a.ldx, gi);
      if (xn != a.x_pad) cx.scatter_add(a.gX + xn * a.ldx, gn);
    }
    if (a.gbi && cx.lane == 0) {
      atomicAdd(a.gbi + ip, g);
      atomicAdd(a.gbi + in, -g);
    }
  }
  const float total = block_sum_waves(part, red);
  if (threadIdx.x == 0 && total != 0.f) atomicAdd(a.loss, total * gmean);
}

struct AlignArgs {
  const float *A, *B;
  int64_t lda, ldb;
  const int64_t *a_ids, *b_ids, *n_dev;
  int64_t cap;
  int d, l1;
  float scale;
  float* loss;
  float *gA, *gB;
};

// One wave per pair, lane j walks columns j, j + 64, ...: each wave instruction of loads and of atomics is 256 contiguous bytes.
__global__ __launch_bounds__(256) void align_pairs_kernel(AlignArgs a) {
  __shared__ float red[4];
  int64_t n = a.n_dev[0];
  n = n < a.cap ? n : a.cap;
  if (n <= 0) return;                                               // (uniform over the grid: nobody waits at the barrier below)
  const float gs = a.scale / (float)n;
  const bool l1 = a.l1 != 0;
  const int lane = threadIdx.x & 63;
  float part = 0.f;
  for (int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); k < n; k += (int64_t)gridDim.x * 4) {
    const int64_t ra = a.a_ids[k] * a.lda, rb = a.b_ids[k] * a.ldb;
    for (int j = lane; j < a.d; j += 64) {
      const float z = a.A[ra + j] - a.B[rb + j];
      part += dist1(z, l1);
      const float g = gs * ddist1(z, l1);
      if (g != 0.f) {
        atomicAdd(a.gA + ra + j, g);
        atomicAdd(a.gB + rb + j, -g);
      }
    }
  }
  const float total = block_sum_waves(group_sum<64>(part), red);
  if (threadIdx.x == 0 && total != 0.f) atomicAdd(a.loss, total * gs);
}

}  // namespace

extern "C" int ktup_train_dot_step_supported(int d) { return (d >= 1 && d <= MAX_D && !opt_deterministic()) ? 1 : 0; }

extern "C" int ktup_train_dot_step(const float* U, int64_t ldu, const float* I, int64_t ldi, const float* X, int64_t ldx,
                                   const int64_t* x_of_item, int64_t x_pad, const float* gbias, const float* bu, const float* bi, int d,
                                   const int64_t* u_ids, const int64_t* i_ids, int64_t B, float target, float up, float* loss, float* gU,
                                   float* gI, float* gX, float* gbi, void* stream) {
  const char* name = "ktup_train_dot_step";
  KTUP_REQUIRE(d >= 1, "%s: embedding_size must be positive (got %d)", name, d);
  KTUP_REQUIRE(B >= 1, "%s: the batch needs at least one example (got %lld)", name, (long long)B);
  KTUP_REQUIRE(U && I && u_ids && i_ids && loss && gU && gI, "%s: null pointer argument", name);
  KTUP_REQUIRE(ldu >= d && ldi >= d, "%s: a row pitch below the width", name);
  KTUP_REQUIRE((X != nullptr) == (x_of_item != nullptr), "%s: the second item-side table and its map come together", name);
  KTUP_REQUIRE(!X || (gX && ldx >= d), "%s: the second item-side table needs its gradient and a pitch >= the width", name);
  if (d > MAX_D) return set_error(KTUP_ERR_UNSUPPORTED, "%s: embedding_size %d is beyond the %d columns a wave holds", name, d, MAX_D);
  if (opt_deterministic())
    return set_error(KTUP_ERR_UNSUPPORTED, "%s: the row gradients are float atomics of many workgroups (option deterministic is set)", name);
  DotStepArgs a{U, I, X, ldu, ldi, ldx, x_of_item, x_pad, gbias, bu, bi, u_ids, i_ids, B, target, up, loss, gU, gI, gX, gbi, 0};
  const bool vec = can_vec4(d, {U, I, X, gU, gI, gX}, {ldu, ldi, X ? ldx : 0});
  const int grid = grid_for((B + 3) / 4);
  hipStream_t st = (hipStream_t)stream;
  if (vec) {
    a.nch = d / 4;                                                  // <= 64: one float4 per lane
    hipLaunchKernelGGL((dot_step_kernel<float4, 1>), dim3(grid), dim3(256), 0, st, a);
  } else {
    a.nch = d;
    if (d <= 64) hipLaunchKernelGGL((dot_step_kernel<float, 1>), dim3(grid), dim3(256), 0, st, a);
    else if (d <= 128) hipLaunchKernelGGL((dot_step_kernel<float, 2>), dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((dot_step_kernel<float, 4>), dim3(grid), dim3(256), 0, st, a);
  }
  return check_launch(name);
}

extern "C" int ktup_reg_align_pairs(const float* A, int64_t lda, const float* B, int64_t ldb, int d, const int64_t* a_ids,
                                    const int64_t* b_ids, const int64_t* n_dev, int64_t n_host, int64_t cap, int l1, float scale,
                                    float* loss, float* gA, float* gB, void* stream) {
  const char* name = "ktup_reg_align_pairs";
  KTUP_REQUIRE(d >= 1, "%s: embedding_size must be positive (got %d)", name, d);
  KTUP_REQUIRE(cap >= 0, "%s: negative capacity", name);
  KTUP_REQUIRE(n_host <= cap, "%s: %lld pairs do not fit the id buffers of capacity %lld", name, (long long)n_host, (long long)cap);
  if (cap == 0 || n_host == 0) return KTUP_OK;
  KTUP_REQUIRE(A && B && a_ids && b_ids && n_dev && loss && gA && gB, "%s: null pointer argument", name);
  KTUP_REQUIRE(lda >= d && ldb >= d, "%s: a row pitch below the width", name);
  AlignArgs a{A, B, lda, ldb, a_ids, b_ids, n_dev, cap, d, l1, scale, loss, gA, gB};
  const int64_t rows = n_host >= 0 ? n_host : cap;
  hipLaunchKernelGGL(align_pairs_kernel, dim3(grid_for((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch(name);
}
