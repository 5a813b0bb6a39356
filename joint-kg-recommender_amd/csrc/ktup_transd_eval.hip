// TransD link prediction: all-entity scores (transD.py:78-134) and the whole filtered-rank pass.
//
// Per key i (query entity q, relation r):  a = Ep[q], b = Rp[r], q_perp = E[q] + (E[q] . a) b,
//     c = q_perp - R[r]  (evaluateHead)   or   q_perp + R[r]  (evaluateTail)
// and every candidate e_j is projected with the QUERY's vector a (transD.py:94-98), so
//     score(i, j) = dist( c - e_j - (e_j . a) b ).
// (evaluateTail of the reference names an undefined t_proj_expand, transD.py:127, and raises NameError; the h_proj_expand it
// computes two lines above -- the query's own projection row -- is the evident intent and what runs here.)
//
// transd_query_prep_kernel writes per key  QW[i] = [c | a | b]  (3 x round4(d) floats, zero tail) and QS[i] = {|c|^2, b.c, |b|^2, 0}.
// Two routes behind ktup_eval_transd_scores:
//   * pair route (L1, any width; squared L2 where the matrix-core route does not apply): 64 candidates staged transposed in
//     LDS (lane <-> candidate, conflict-free b128 reads), the four waves of a workgroup take different keys, QB = 4 at a time,
//     whose vectors arrive through scalar loads.  Pass 1: s = e . a, pass 2: sum dist(c - e - s b) -- the direct form.
//   * matrix-core route (squared L2, d in {20, 36, 64, 100, 128}): the score expands into three (keys x candidates) products,
//         |c - e - (e.a) b|^2 = |c|^2 - 2 [c.e] + |e|^2 - 2 [a.e] (b.c - [b.e]) + [a.e]^2 |b|^2,
//     all three formed per 64 x 64 tile on v_mfma_f32_16x16x4_f32 with fp32 accumulation.  [b.e] depends on (relation, candidate)
//     only; it is still a third product per tile rather than a relation x candidate table built once per call: the kernel is
//     bound by writing the score matrix, not by the matrix cores, the b rows ride in the stage the c and a rows need anyway, and a
//     table would cost a launch, n_rel x n_cand floats of workspace, a relation-id gather in the epilogue and would tie the
//     candidate slice of a sharded pass to a per-slice table.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ktup_common.h"
#include "ktup_lane_swap.h"
#include "ktup_pref_geom.h"

using namespace ktup;

namespace {

constexpr int CT = 64;   // candidates per workgroup tile
constexpr int QB = 4;    // keys a wave scores together (each LDS read serves QB keys)
constexpr int NWV = 4;   // waves per workgroup of the pair kernel

inline int round4(int d) { return (d + 3) / 4 * 4; }
inline size_t qw_floats(int d, int64_t nq) { return (size_t)nq * 3 * round4(d); }

// One wave per key.
__global__ __launch_bounds__(256) void transd_query_prep_kernel(const float* __restrict__ E, int64_t lde, const float* __restrict__ Ep,
                                                                int64_t ldep, const float* __restrict__ R, int64_t ldr,
                                                                const float* __restrict__ Rp, int64_t ldrp, int d, int dq,
                                                                const int64_t* __restrict__ q, const int64_t* __restrict__ r, int64_t nq,
                                                                int head, float* __restrict__ QW, float* __restrict__ QS) {
  const int lane = threadIdx.x & 63;
  const float sgn = head ? -1.f : 1.f;
  for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < nq; i += (int64_t)gridDim.x * 4) {
    const float* e = E + q[i] * lde;
    const float* a = Ep + q[i] * ldep;
    const float* rel = R + r[i] * ldr;
    const float* b = Rp + r[i] * ldrp;
    float* out = QW + i * 3 * dq;
    float dot = 0.f;
    for (int k = lane; k < d; k += 64) dot = fmaf(e[k], a[k], dot);
    dot = group_sum<64>(dot);
    float cc = 0.f, bc = 0.f, bb = 0.f;
    for (int k = lane; k < dq; k += 64) {
      float c = 0.f, av = 0.f, bv = 0.f;
      if (k < d) { av = a[k]; bv = b[k]; c = fmaf(dot, bv, e[k]) + sgn * rel[k]; }
      out[k] = c; out[dq + k] = av; out[2 * dq + k] = bv;
      cc = fmaf(c, c, cc); bc = fmaf(bv, c, bc); bb = fmaf(bv, bv, bb);
    }
    cc = group_sum<64>(cc); bc = group_sum<64>(bc); bb = group_sum<64>(bb);
    if (lane == 0) { QS[i * 4 + 0] = cc; QS[i * 4 + 1] = bc; QS[i * 4 + 2] = bb; QS[i * 4 + 3] = 0.f; }
  }
}

// ------------------------------------------------------------------------------------------------------------ pair route
struct PairArgs {
  const float* C; int64_t ldc; int64_t n_cand;
  const float* QW; int64_t nq;
  int d, dq; bool cvec;
  float* out; int64_t ldo;
};

typedef float v2f __attribute__((ext_vector_type(2)));
KTUP_DEV v2f lo2(float4 a) { return v2f{a.x, a.y}; }
KTUP_DEV v2f hi2(float4 a) { return v2f{a.z, a.w}; }
KTUP_DEV v2f fma2(v2f a, v2f b, v2f c) { return __builtin_elementwise_fma(a, b, c); }

KTUP_DEV float4 load_cand4(const float* base, int64_t ld, int64_t row, int c, int d, bool vec) {
  const float* p = base + row * ld + 4 * c;
  if (vec) return *reinterpret_cast<const float4*>(p);
  float4 v;
  v.x = 4 * c + 0 < d ? p[0] : 0.f;
  v.y = 4 * c + 1 < d ? p[1] : 0.f;
  v.z = 4 * c + 2 < d ? p[2] : 0.f;
  v.w = 4 * c + 3 < d ? p[3] : 0.f;
  return v;
}

template <bool L1>
__global__ __launch_bounds__(NWV * 64) void transd_pairs_kernel(PairArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4* cand = reinterpret_cast<float4*>(smem);          // [nch4][CT]
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int nch4 = a.dq / 4;
  const int64_t j0 = (int64_t)blockIdx.x * CT;
  for (int idx = t; idx < nch4 * CT; idx += NWV * 64) {
    const int j = idx & (CT - 1), c = idx >> 6;
    const int64_t gj = min(j0 + j, a.n_cand - 1);            // (rows past the end repeat the last one; never stored)
    cand[c * CT + j] = load_cand4(a.C, a.ldc, gj, c, a.d, a.cvec);
  }
  __syncthreads();
  const sptr4 QW = as_scalar(a.QW);
  // this workgroup's slice of the keys (grid.y splits them), QB at a time per wave
  const int64_t per = ((a.nq + gridDim.y - 1) / gridDim.y + NWV * QB - 1) / (NWV * QB) * (NWV * QB);
  const int64_t qlo = (int64_t)blockIdx.y * per, qhi = min(a.nq, qlo + per);
  for (int64_t b0 = qlo + w * QB; b0 < qhi; b0 += NWV * QB) {
    sptr4 qc[QB], qa[QB], qb[QB];
#pragma unroll
    for (int qi = 0; qi < QB; ++qi) {
      const int64_t pos = min(b0 + qi, a.nq - 1);
      qc[qi] = QW + pos * 3 * nch4;
      qa[qi] = qc[qi] + nch4;
      qb[qi] = qc[qi] + 2 * nch4;
    }
    v2f s2[QB], a2[QB];
    float acc[QB];
#pragma unroll
    for (int qi = 0; qi < QB; ++qi) { s2[qi] = v2f{0.f, 0.f}; a2[qi] = v2f{0.f, 0.f}; acc[qi] = 0.f; }
#pragma unroll 2
    for (uint32_t c = 0; c < (uint32_t)nch4; ++c) {          // pass 1: -(e . a)
      const float4 e = cand[c * CT + lane];
#pragma unroll
      for (int qi = 0; qi < QB; ++qi) {
        const float4 av = sldp(qa[qi] + c);
        s2[qi] = fma2(-lo2(e), lo2(av), s2[qi]);
        s2[qi] = fma2(-hi2(e), hi2(av), s2[qi]);
      }
    }
    v2f ms[QB];
#pragma unroll
    for (int qi = 0; qi < QB; ++qi) { const float s = s2[qi].x + s2[qi].y; ms[qi] = v2f{s, s}; }
#pragma unroll 2
    for (uint32_t c = 0; c < (uint32_t)nch4; ++c) {          // pass 2: z = (c - e) - (e . a) b
      const float4 e = cand[c * CT + lane];
#pragma unroll
      for (int qi = 0; qi < QB; ++qi) {
        const float4 cv = sldp(qc[qi] + c), bv = sldp(qb[qi] + c);
        const v2f zl = fma2(ms[qi], lo2(bv), lo2(cv) - lo2(e)), zh = fma2(ms[qi], hi2(bv), hi2(cv) - hi2(e));
        if constexpr (L1) {
          acc[qi] += (fabsf(zl.x) + fabsf(zl.y)) + (fabsf(zh.x) + fabsf(zh.y));
        } else {
          a2[qi] = fma2(zl, zl, a2[qi]);
          a2[qi] = fma2(zh, zh, a2[qi]);
        }
      }
    }
    if (j0 + lane < a.n_cand) {
#pragma unroll
      for (int qi = 0; qi < QB; ++qi)
        if (b0 + qi < qhi) a.out[(b0 + qi) * a.ldo + j0 + lane] = L1 ? acc[qi] : a2[qi].x + a2[qi].y;
    }
  }
}

// grid.y splits the keys: about `target` workgroups for a short call, up to 8 rounds of the chip's slots for a long one, every
// split a whole number of NWV x QB key groups.
dim3 pairs_grid(int64_t n_cand, int64_t nq) {
  const int64_t tiles = (n_cand + CT - 1) / CT, group = NWV * QB, slots = 1536;
  const int64_t ymax = (nq + group - 1) / group;
  int64_t target = 2048;
  const int64_t fine = tiles * ymax / 6;
  if (fine > target) target = fine < 8 * slots ? fine : 8 * slots;
  int64_t ysplit = (target + tiles - 1) / tiles;
  if (ysplit > ymax) ysplit = ymax;
  if (ysplit < 1) ysplit = 1;
  const int64_t per = ((nq + ysplit - 1) / ysplit + group - 1) / group * group;
  ysplit = (nq + per - 1) / per;
  return dim3((unsigned)tiles, (unsigned)(ysplit < 1 ? 1 : ysplit));
}

int launch_pairs(const PairArgs& a, int l1, hipStream_t st, const char* name) {
  const size_t lds = (size_t)(a.dq / 4) * CT * 16;
  if (lds > 160 * 1024) return set_error(KTUP_ERR_UNSUPPORTED, "%s: embedding_size %d needs %zu B of LDS", name, a.d, lds);
  const dim3 grid = pairs_grid(a.n_cand, a.nq);
  if (grid.y > 65535) return set_error(KTUP_ERR_UNSUPPORTED, "%s: too many keys for one call (%lld)", name, (long long)a.nq);
  if (l1) {
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)transd_pairs_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(transd_pairs_kernel<true>, grid, dim3(NWV * 64), lds, st, a);
  } else {
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)transd_pairs_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(transd_pairs_kernel<false>, grid, dim3(NWV * 64), lds, st, a);
  }
  return check_launch(name);
}

// ------------------------------------------------------------------------------------------------------ matrix-core route
constexpr int IB = 64;   // candidates per workgroup

template <int NCH_>
struct DGeom {
  static constexpr int NCH = NCH_, D = 4 * NCH;
  static constexpr int KG = (D + 15) / 16;
  static constexpr bool TAIL1 = NCH - 4 * (KG - 1) == 1;       // d % 16 == 4: the last chunk goes through one b32-operand MFMA
  static constexpr int KGF = TAIL1 ? KG - 1 : KG;
  static_assert(TAIL1 || NCH % 4 == 0, "k groups must be whole (d % 16 in {0, 4})");
  static constexpr int P4 = NCH | 1;                           // odd float4 row pitch: conflict-free b128 operand reads
  static constexpr int QV = 3;                                 // vectors per key: c, a, b
  static constexpr int UB = 64, NW = 16;
  static constexpr size_t LDS = (size_t)(UB * QV + IB) * P4 * 16 + (size_t)IB * 4;
  static_assert(LDS <= 160 * 1024, "LDS budget");
};

struct McArgs {
  const float* QW; const float* QS;
  const float* C; int64_t ldc;
  int64_t nq, n_cand;
  float* out; int64_t ldo;
};

template <typename G>
__global__ __launch_bounds__(G::NW * 64) void transd_l2_mc_kernel(McArgs a) {
  constexpr int NCH = G::NCH, UB = G::UB, KGF = G::KGF, P4 = G::P4, NW = G::NW, QV = G::QV, D = G::D;
  constexpr bool TAIL1 = G::TAIL1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  v4* Q = reinterpret_cast<v4*>(smem);                         // [UB][QV][P4]
  v4* Cd = Q + UB * QV * P4;                                   // [IB][P4]
  float* cs = reinterpret_cast<float*>(Cd + IB * P4);          // [IB]: |e|^2
  const int tid = threadIdx.x, lane = tid & 63, kq = lane >> 4, j = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  // XCD-aware tile order: consecutive workgroups go round-robin to the 8 XCDs; each XCD gets a contiguous band of candidate
  // tiles, so its L2 holds its band and the (small) key block.  grid.x is padded to 8 bands of nxp tiles.
  const int nxp = gridDim.x >> 3;
  const int bid = blockIdx.y * gridDim.x + blockIdx.x, xcd = bid & 7, local = bid >> 3;
  const int tx = xcd * nxp + local % nxp, ty = local / nxp;
  if ((int64_t)tx * IB >= a.n_cand) return;
  const int64_t u0 = (int64_t)ty * UB, i0 = (int64_t)tx * IB;
  for (int idx = tid; idx < UB * QV * NCH; idx += NW * 64) {
    const int row = idx / (QV * NCH), rem = idx - row * (QV * NCH), vec = rem / NCH, c = rem - vec * NCH;
    v4 val = (v4){0.f, 0.f, 0.f, 0.f};
    if (u0 + row < a.nq) val = *reinterpret_cast<const v4*>(a.QW + ((u0 + row) * 3 + vec) * D + 4 * c);
    Q[(row * QV + vec) * P4 + c] = val;
  }
  for (int idx = tid; idx < IB * NCH; idx += NW * 64) {
    const int row = idx / NCH, c = idx - row * NCH;
    v4 val = (v4){0.f, 0.f, 0.f, 0.f};
    if (i0 + row < a.n_cand) val = *reinterpret_cast<const v4*>(a.C + (i0 + row) * a.ldc + 4 * c);
    Cd[row * P4 + c] = val;
  }
  __syncthreads();
  for (int row = tid >> 3; row < IB; row += (NW * 64) >> 3) {  // |e|^2, 8 lanes per candidate
    const v4* r0 = Cd + row * P4;
    v4 s0 = (v4){0.f, 0.f, 0.f, 0.f};
    for (int c = tid & 7; c < NCH; c += 8) { const v4 x0 = r0[c]; s0 += x0 * x0; }
    float f0 = (s0[0] + s0[1]) + (s0[2] + s0[3]);
#pragma unroll
    for (int m = 1; m < 8; m <<= 1) f0 += __shfl_xor(f0, m, 64);
    if ((tid & 7) == 0) cs[row] = f0;
  }
  __syncthreads();
  // this wave's 16 x 16 tile: keys are MFMA rows (A operand), candidates columns (B operand)
  const int ut = w >> 2, it = w & 3;
  const v4* qa = Q + ((16 * ut + j) * QV) * P4 + kq;           // lane (kq, row j): c at +0, a at +P4, b at +2 P4
  const v4* cb = Cd + (16 * it + j) * P4 + kq;
  v4 ce = (v4){0.f, 0.f, 0.f, 0.f}, ae = ce, be = ce;
#pragma unroll
  for (int g = 0; g < KGF; ++g) {
    const v4 xc = qa[4 * g], xa = qa[P4 + 4 * g], xb = qa[2 * P4 + 4 * g], xe = cb[4 * g];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      ce = __builtin_amdgcn_mfma_f32_16x16x4f32(xc[c], xe[c], ce, 0, 0, 0);
      ae = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[c], xe[c], ae, 0, 0, 0);
      be = __builtin_amdgcn_mfma_f32_16x16x4f32(xb[c], xe[c], be, 0, 0, 0);
    }
  }
  if (TAIL1) {                                                 // coordinates 16 KGF + kq
    const float* qf = reinterpret_cast<const float*>(Q + ((16 * ut + j) * QV) * P4 + 4 * KGF) + kq;
    const float xe = (reinterpret_cast<const float*>(Cd + (16 * it + j) * P4 + 4 * KGF) + kq)[0];
    ce = __builtin_amdgcn_mfma_f32_16x16x4f32(qf[0], xe, ce, 0, 0, 0);
    ae = __builtin_amdgcn_mfma_f32_16x16x4f32(qf[4 * P4], xe, ae, 0, 0, 0);
    be = __builtin_amdgcn_mfma_f32_16x16x4f32(qf[8 * P4], xe, be, 0, 0, 0);
  }
  // epilogue: lane (kq, j) holds keys 16 ut + 4 kq + reg (reg = 0..3) x candidate 16 it + j
  const float ee = cs[16 * it + j];
  const int64_t cnd = i0 + 16 * it + j;
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int64_t key = u0 + 16 * ut + 4 * kq + reg;
    if (key < a.nq && cnd < a.n_cand) {
      const v4 qs = *reinterpret_cast<const v4*>(a.QS + key * 4);       // |c|^2, b.c, |b|^2
      const float s = ae[reg];
      float score = fmaf(-2.f, ce[reg], qs[0] + ee);
      score = fmaf(s, fmaf(s, qs[2], -2.f * (qs[1] - be[reg])), score);
      a.out[key * a.ldo + cnd] = score;
    }
  }
}

template <typename G>
int launch_mc(const McArgs& a, hipStream_t st, const char* name) {
  (void)hipFuncSetAttribute((const void*)transd_l2_mc_kernel<G>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)G::LDS);
  const unsigned nx = (unsigned)((a.n_cand + IB - 1) / IB), nxp = (nx + 7) / 8;       // 8 XCD bands of nxp candidate tiles
  const dim3 grid(8 * nxp, (unsigned)((a.nq + G::UB - 1) / G::UB));
  hipLaunchKernelGGL((transd_l2_mc_kernel<G>), grid, dim3(G::NW * 64), G::LDS, st, a);
  return check_launch(name);
}

// KTUP_OK / an error, or 1 when the shape is not one of the instantiated ones (the caller runs the pair kernel).
int transd_l2_mc(const McArgs& a, int d, int dq, hipStream_t st, const char* name) {
  if (!aligned16(a.QW) || !aligned16(a.QS) || !aligned16(a.C) || (a.ldc & 3) || dq != d) return 1;
  if ((a.nq + 63) / 64 > 65535) return 1;
  switch (d) {
    case 20: return launch_mc<DGeom<5>>(a, st, name);
    case 36: return launch_mc<DGeom<9>>(a, st, name);
    case 64: return launch_mc<DGeom<16>>(a, st, name);
    case 100: return launch_mc<DGeom<25>>(a, st, name);
    case 128: return launch_mc<DGeom<32>>(a, st, name);
    default: return 1;
  }
}

size_t score_bytes(int64_t chunk, int64_t n_cand) { return (((size_t)chunk * (size_t)n_cand * sizeof(float)) + 255) & ~(size_t)255; }

// double-buffered pass: the rank kernel of chunk c on the library's side stream beside the score kernel of chunk c + 1
struct Ev {
  hipEvent_t ready[2] = {nullptr, nullptr}, done[2] = {nullptr, nullptr};
  bool tried = false, ok = false;
} g_ev;

bool events_ok() {
  if (!g_ev.tried) {
    g_ev.tried = true;
    g_ev.ok = true;
    for (int i = 0; i < 2; ++i)
      if (hipEventCreateWithFlags(&g_ev.ready[i], hipEventDisableTiming) != hipSuccess ||
          hipEventCreateWithFlags(&g_ev.done[i], hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        g_ev.ok = false;
      }
  }
  return g_ev.ok;
}

}  // namespace

extern "C" size_t ktup_eval_transd_workspace_bytes(int d, int64_t nq) {
  if (d <= 0 || nq <= 0) return 0;
  return (qw_floats(d, nq) + (size_t)nq * 4) * sizeof(float);
}

extern "C" int ktup_eval_transd_scores(const float* E, int64_t lde, const float* Ep, int64_t ldep, const float* R, int64_t ldr,
                                       const float* Rp, int64_t ldrp, int d, const float* C, int64_t ldc, int64_t n_cand,
                                       const int64_t* q, const int64_t* r, int64_t nq, int l1, int head, float* out, int64_t ldo,
                                       float* ws, void* stream) {
  const char* name = "ktup_eval_transd_scores";
  KTUP_REQUIRE(d > 0 && nq >= 0 && n_cand >= 0, "%s: bad sizes", name);
  if (nq == 0 || n_cand == 0) return KTUP_OK;
  KTUP_REQUIRE(E && Ep && R && Rp && C && q && r && out && ws, "%s: null pointer argument", name);
  KTUP_REQUIRE(ldo >= n_cand, "%s: output pitch %lld < n_cand", name, (long long)ldo);
  KTUP_REQUIRE(aligned16(ws), "%s: workspace must be 16-byte aligned", name);
  hipStream_t st = (hipStream_t)stream;
  const int dq = round4(d);
  float* QW = ws;
  float* QS = ws + qw_floats(d, nq);
  hipLaunchKernelGGL(transd_query_prep_kernel, dim3(grid_for((nq + 3) / 4)), dim3(256), 0, st, E, lde, Ep, ldep, R, ldr, Rp, ldrp, d, dq,
                     q, r, nq, head, QW, QS);
  if (int e = check_launch(name)) return e;
  if (!l1 && ktup::opt_eval_mc()) {
    const McArgs m{QW, QS, C, ldc, nq, n_cand, out, ldo};
    const int rc = transd_l2_mc(m, d, dq, st, name);
    if (rc != 1) return rc;
  }
  PairArgs a{};
  a.C = C; a.ldc = ldc; a.n_cand = n_cand; a.QW = QW; a.nq = nq; a.d = d; a.dq = dq; a.out = out; a.ldo = ldo;
  a.cvec = (d % 4 == 0) && aligned16(C) && (ldc % 4 == 0);
  return launch_pairs(a, l1, st, name);
}

extern "C" size_t ktup_eval_kg_ranks_transd_workspace_bytes(int d, int64_t n_cand, int64_t chunk) {
  if (d <= 0 || n_cand <= 0 || chunk <= 0) return 0;
  return 2 * score_bytes(chunk, n_cand) + ktup_eval_transd_workspace_bytes(d, chunk);
}

extern "C" int ktup_eval_kg_ranks_transd(const float* E, int64_t lde, const float* Ep, int64_t ldep, const float* R, int64_t ldr,
                                         const float* Rp, int64_t ldrp, int d, const float* C, int64_t ldc, int64_t n_cand,
                                         const int64_t* q, const int64_t* r, int64_t nq, int l1, int head, int descending,
                                         const int64_t* filt_off, const int32_t* filt_ids, const int64_t* gold_off,
                                         const int32_t* gold_ids, int32_t* ranks, int64_t chunk, void* ws, void* stream) {
  const char* name = "ktup_eval_kg_ranks_transd";
  KTUP_REQUIRE(nq >= 0 && n_cand > 0 && chunk > 0 && d > 0, "%s: bad sizes", name);
  if (nq == 0) return KTUP_OK;
  KTUP_REQUIRE(E && Ep && R && Rp && C && q && r && gold_off && gold_ids && ranks && ws, "%s: null pointer argument", name);
  KTUP_REQUIRE((filt_off == nullptr) || filt_ids, "%s: filter offsets without ids", name);
  KTUP_REQUIRE(aligned16(ws), "%s: workspace must be 16-byte aligned", name);
  hipStream_t st = (hipStream_t)stream;
  const size_t sb = score_bytes(chunk, n_cand) / sizeof(float);
  float* scores2 = reinterpret_cast<float*>(ws);
  float* qws = scores2 + 2 * sb;
  // The key-side scratch is rewritten per chunk.  With the side stream only the RANK kernel of a chunk runs there; the prep and score
  // kernels of all chunks stay in order on `st`, so the scratch is never rewritten while a score kernel reads it.
  hipStream_t side = (nq > chunk && events_ok()) ? ktup::fork_side(st) : nullptr;
  int64_t c = 0;
  for (int64_t c0 = 0; c0 < nq; c0 += chunk, ++c) {
    const int64_t nb = nq - c0 < chunk ? nq - c0 : chunk;
    const int b = (int)(c & 1);
    float* out = scores2 + (side ? b * sb : 0);
    if (side && c >= 2 && hipStreamWaitEvent(st, g_ev.done[b], 0) != hipSuccess) return ktup::check_launch(name);   // ranks(c - 2) has read this buffer
    int rc = ktup_eval_transd_scores(E, lde, Ep, ldep, R, ldr, Rp, ldrp, d, C, ldc, n_cand, q + c0, r + c0, nb, l1, head, out, n_cand, qws, st);
    if (rc != KTUP_OK) { ktup::join_side(st, side); return rc; }
    hipStream_t rs = st;
    if (side) {
      if (hipEventRecord(g_ev.ready[b], st) != hipSuccess || hipStreamWaitEvent(side, g_ev.ready[b], 0) != hipSuccess) return ktup::check_launch(name);
      rs = side;
    }
    rc = ktup_eval_gold_ranks(out, n_cand, nb, n_cand, descending, filt_off ? filt_off + c0 : nullptr, filt_ids, gold_off + c0, gold_ids, ranks, rs);
    if (rc != KTUP_OK) { ktup::join_side(st, side); return rc; }
    if (side && hipEventRecord(g_ev.done[b], side) != hipSuccess) return ktup::check_launch(name);
  }
  ktup::join_side(st, side);                   // the caller's stream continues after the last rank kernel
  return KTUP_OK;
}
