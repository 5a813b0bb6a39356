// The TransD training step of the KG driver as ONE launch (knowledge_representation.py:176-204 with transD.py:61-76): a sibling of
// kg_step_kernel (ktup_train_step.hip) with two more tables.  A lane group owns example k = the positive triple k and its corrupted
// twin k + B and holds their twelve rows (h, t, h_p, t_p, r, r_p of each; the twin's relation may differ) in registers as float4:
//   alpha = h . h_p,  beta = t . t_p,  v = (h + alpha r_p) + r - (t + beta r_p),  s = sum |v| or sum v^2       (ktup_score_transd_fwd)
//   marginLoss: sum_k max(s+ - s- + margin, 0);  normLoss(entity rows), normLoss(relation rows) from the rows in registers
//   g = +-gscale dist'(v) of an active example, gamma = g . r_p:
//   gE[h] += g + gamma h_p   gEp[h] += gamma h   gE[t] -= g + gamma t_p   gEp[t] -= gamma t   gR[r] += g   gRp[r] += (alpha - beta) g
// Each gathered row receives one float4 atomic per chunk with the sum of its contributions; a row that receives nothing (an inactive
// example's projection rows, its entity and relation rows unless their regulariser fires) gets no atomic at all.  Ep and Rp carry no
// regulariser (knowledge_representation.py:200-204).
#include "ktup_common.h"

using namespace ktup;

namespace {

struct TdStepArgs {
  const float *E, *R, *Ep, *Rp; int64_t lde, ldr, ldep, ldrp;
  const int64_t *h, *t, *r;      // [pos ; neg] rows: k and k + B
  int64_t B; int nch; bool l1;
  float margin, gscale;
  int regs;                      // bit 1 normLoss(entity rows), bit 2 normLoss(relation rows)
  float* loss;                   // [4]: margin sum, (unused), normE, normR  (accumulated)
  float *gE, *gR, *gEp, *gRp;
  double* gnorm;                 // (may be null) the gradient-norm workspace of ktup_common.h
  int serial;                    // option `deterministic`: one lane group of one workgroup walks every example (kg_step_kernel)
};

template <int GL>
__global__ __launch_bounds__(256) void transd_step_kernel(TdStepArgs a) {
  constexpr int GPB = 256 / GL;
  const int lane = threadIdx.x % GL;
  const bool on = lane < a.nch;
  float part[4] = {0.f, 0.f, 0.f, 0.f};
  const float g1 = a.gscale;
  const bool track = a.gnorm != nullptr;
  const int gset = track ? gnorm_set(a.gnorm) : 0;
  float ssq = 0.f;
  const int64_t k0 = a.serial ? (threadIdx.x < GL ? 0 : a.B) : (int64_t)blockIdx.x * GPB + threadIdx.x / GL;
  const int64_t kstep = a.serial ? 1 : (int64_t)gridDim.x * GPB;
  for (int64_t k = k0; k < a.B; k += kstep) {
    const int64_t id[4] = {a.h[k], a.t[k], a.h[k + a.B], a.t[k + a.B]};      // ph, pt, nh, nt
    const int64_t rid[2] = {a.r[k], a.r[k + a.B]};
    float4 e[4], ep[4], rr[2], rp[2];
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      e[x] = on ? reinterpret_cast<const float4*>(a.E + id[x] * a.lde)[lane] : f4zero();
      ep[x] = on ? reinterpret_cast<const float4*>(a.Ep + id[x] * a.ldep)[lane] : f4zero();
    }
#pragma unroll
    for (int x = 0; x < 2; ++x) {
      rr[x] = on ? reinterpret_cast<const float4*>(a.R + rid[x] * a.ldr)[lane] : f4zero();
      rp[x] = on ? reinterpret_cast<const float4*>(a.Rp + rid[x] * a.ldrp)[lane] : f4zero();
    }
    // ---- forward of both triples, in the order of ktup_score_transd_fwd: e + (e . e_p) r_p, then h + r - t
    float ab[2], sc[2];
    float4 v[2];
#pragma unroll
    for (int x = 0; x < 2; ++x) {
      const float al = group_sum<GL>(dot4(e[2 * x], ep[2 * x]));
      const float be = group_sum<GL>(dot4(e[2 * x + 1], ep[2 * x + 1]));
      const float4 hp = fma4(al, rp[x], e[2 * x]), tp = fma4(be, rp[x], e[2 * x + 1]);
      v[x] = (hp + rr[x]) - tp;
      ab[x] = al - be;
      sc[x] = group_sum<GL>(dist4(v[x], a.l1));
    }
    // ---- marginLoss (utils/loss.py:8-16): sum_k max(pos - neg + margin, 0)
    const float diff = sc[0] - sc[1];
    const bool act = diff + a.margin > 0.f;
    if (lane == 0) part[0] += fmaxf(diff + a.margin, 0.f);
    // ---- backward of both triples + the regularisers of the rows in registers
    float4 ge[4], gep[4], gr[2], grp[2];
    bool he[4] = {act, act, act, act}, hr[2] = {act, act};     // rows that receive something (uniform over the lane group)
#pragma unroll
    for (int x = 0; x < 2; ++x) {
      const float4 g = (act ? (x == 0 ? g1 : -g1) : 0.f) * ddist4(v[x], a.l1);
      const float gam = group_sum<GL>(dot4(g, rp[x]));
      ge[2 * x] = fma4(gam, ep[2 * x], g);
      ge[2 * x + 1] = -1.f * fma4(gam, ep[2 * x + 1], g);
      gep[2 * x] = gam * e[2 * x];
      gep[2 * x + 1] = (-gam) * e[2 * x + 1];
      gr[x] = g;
      grp[x] = ab[x] * g;
    }
    if (a.regs & 2) {                 // normLoss(ent rows): sum max(|x|^2 - 1, 0)  (utils/loss.py:21-23)
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const float s = group_sum<GL>(dot4(e[x], e[x]));
        if (s - 1.f > 0.f) { ge[x] = fma4(2.f * g1, e[x], ge[x]); he[x] = true; }
        if (lane == 0) part[2] += fmaxf(s - 1.f, 0.f);
      }
    }
    if (a.regs & 4) {                 // normLoss(rel rows)
#pragma unroll
      for (int x = 0; x < 2; ++x) {
        const float s = group_sum<GL>(dot4(rr[x], rr[x]));
        if (s - 1.f > 0.f) { gr[x] = fma4(2.f * g1, rr[x], gr[x]); hr[x] = true; }
        if (lane == 0) part[3] += fmaxf(s - 1.f, 0.f);
      }
    }
    if (on && track) {                // every add issued before the first returned value is used (ktup_common.h)
      float4 oe[4], oep[4], orr[2], orp[2];
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        oe[x] = he[x] ? atomic_add4_old(a.gE + id[x] * a.lde + 4 * lane, ge[x]) : f4zero();
        oep[x] = act ? atomic_add4_old(a.gEp + id[x] * a.ldep + 4 * lane, gep[x]) : f4zero();
      }
#pragma unroll
      for (int x = 0; x < 2; ++x) {
        orr[x] = hr[x] ? atomic_add4_old(a.gR + rid[x] * a.ldr + 4 * lane, gr[x]) : f4zero();
        orp[x] = act ? atomic_add4_old(a.gRp + rid[x] * a.ldrp + 4 * lane, grp[x]) : f4zero();
      }
#pragma unroll
      for (int x = 0; x < 4; ++x) ssq += (he[x] ? sq_gain4(oe[x], ge[x]) : 0.f) + (act ? sq_gain4(oep[x], gep[x]) : 0.f);
#pragma unroll
      for (int x = 0; x < 2; ++x) ssq += (hr[x] ? sq_gain4(orr[x], gr[x]) : 0.f) + (act ? sq_gain4(orp[x], grp[x]) : 0.f);
    } else if (on) {
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        if (he[x]) atomic_add4(a.gE + id[x] * a.lde + 4 * lane, ge[x]);
        if (act) atomic_add4(a.gEp + id[x] * a.ldep + 4 * lane, gep[x]);
      }
#pragma unroll
      for (int x = 0; x < 2; ++x) {
        if (hr[x]) atomic_add4(a.gR + rid[x] * a.ldr + 4 * lane, gr[x]);
        if (act) atomic_add4(a.gRp + rid[x] * a.ldrp + 4 * lane, grp[x]);
      }
    }
  }
  // ---- the loss values: wave sums -> one atomic per workgroup and slot (slot 1 stays 0 and is never written)
  __shared__ float red[4][5];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const float w = group_sum<64>(part[s]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][s] = w;
  }
  if (track) {
    ssq = group_sum<64>(ssq);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][4] = ssq;
  }
  __syncthreads();
  if (track && threadIdx.x == 64) gnorm_add(a.gnorm, gset, ((double)red[0][4] + (double)red[1][4]) + ((double)red[2][4] + (double)red[3][4]));
  if (threadIdx.x < 4) {
    const float w = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    if (w != 0.f) atomicAdd(a.loss + threadIdx.x, w);
  }
}

int launch_transd(const TdStepArgs& a, hipStream_t st, const char* name) {
#define KTUP_TDS(GL)                                                                                           \
  {                                                                                                            \
    const int grid = a.serial ? 1 : grid_for((a.B + (256 / GL) - 1) / (256 / GL), 1024);                       \
    hipLaunchKernelGGL((transd_step_kernel<GL>), dim3(grid), dim3(256), 0, st, a);                             \
    return check_launch(name);                                                                                 \
  }
  if (a.nch <= 16) KTUP_TDS(16)
  if (a.nch <= 32) KTUP_TDS(32)
  KTUP_TDS(64)
#undef KTUP_TDS
}

}  // namespace

#define KTUP_TDS_NONNULL(p) KTUP_REQUIRE((p) != nullptr, "%s: null pointer argument '" #p "'", name)

extern "C" int ktup_train_transd_step_supported(int d) { return d >= 1 && d <= 256 && d % 4 == 0; }

extern "C" int ktup_train_transd_step(const float* E, int64_t lde, const float* R, int64_t ldr, const float* Ep, int64_t ldep,
                                      const float* Rp, int64_t ldrp, int d, const int64_t* h, const int64_t* t, const int64_t* r,
                                      int64_t B, int l1, float margin, float gscale, int regs, float* loss, float* gE, float* gR,
                                      float* gEp, float* gRp, double* gnorm, void* stream) {
  const char* name = "ktup_train_transd_step";
  KTUP_REQUIRE(d > 0, "%s: embedding_size must be positive (got %d)", name, d);
  KTUP_REQUIRE(B >= 0 && (B > 0 || !gnorm), "%s: negative batch (or an empty one with a tracked norm)", name);
  KTUP_REQUIRE((regs & ~6) == 0, "%s: regs takes bit 1 (normLoss of the entity rows) and bit 2 (normLoss of the relation rows); TransD has no "
               "orthogonalLoss (bit 0)", name);
  if (B == 0) return KTUP_OK;
  KTUP_TDS_NONNULL(E); KTUP_TDS_NONNULL(R); KTUP_TDS_NONNULL(Ep); KTUP_TDS_NONNULL(Rp);
  KTUP_TDS_NONNULL(h); KTUP_TDS_NONNULL(t); KTUP_TDS_NONNULL(r); KTUP_TDS_NONNULL(loss);
  KTUP_TDS_NONNULL(gE); KTUP_TDS_NONNULL(gR); KTUP_TDS_NONNULL(gEp); KTUP_TDS_NONNULL(gRp);
  if (!ktup_train_transd_step_supported(d) || (lde | ldr | ldep | ldrp) % 4 || !aligned16(E) || !aligned16(R) || !aligned16(Ep) || !aligned16(Rp) ||
      !aligned16(gE) || !aligned16(gR) || !aligned16(gEp) || !aligned16(gRp))
    return set_error(KTUP_ERR_UNSUPPORTED, "%s: needs d %% 4 == 0 (<= 256; got %d) and 16-byte aligned tables and gradients with pitches that are "
                     "multiples of 4 floats (see ktup_train_transd_step_supported)", name, d);
  TdStepArgs a{E, R, Ep, Rp, lde, ldr, ldep, ldrp, h, t, r, B, d / 4, l1 != 0, margin, gscale, regs, loss, gE, gR, gEp, gRp, gnorm,
               opt_deterministic() != 0};
  return launch_transd(a, (hipStream_t)stream, name);
}
