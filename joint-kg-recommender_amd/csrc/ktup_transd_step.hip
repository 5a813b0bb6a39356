// The TransD training step of the KG driver as ONE launch (knowledge_representation.py:176-204 with transD.py:61-76): built from
// the parts of ktup_kg_pair.h that kg_step_kernel (ktup_train_step.hip) is built from -- the walk over the examples, normLoss over rows in
// registers, the scatter's two forms, the workgroup tail -- around its own arithmetic on two more tables.  A lane group owns example k = the positive triple k and its corrupted
// twin k + B and holds their twelve rows (h, t, h_p, t_p, r, r_p of each; the twin's relation may differ) in registers as float4:
//   alpha = h . h_p,  beta = t . t_p,  v = (h + alpha r_p) + r - (t + beta r_p),  s = sum |v| or sum v^2       (ktup_score_transd_fwd)
//   marginLoss: sum_k max(s+ - s- + margin, 0);  normLoss(entity rows), normLoss(relation rows) from the rows in registers
//   g = +-gscale dist'(v) of an active example, gamma = g . r_p:
//   gE[h] += g + gamma h_p   gEp[h] += gamma h   gE[t] -= g + gamma t_p   gEp[t] -= gamma t   gR[r] += g   gRp[r] += (alpha - beta) g
// Each gathered row receives one float4 atomic per chunk with the sum of its contributions; a row that receives nothing (an inactive
// example's projection rows, its entity and relation rows unless their regulariser fires) gets no atomic at all.  Ep and Rp carry no
// regulariser (knowledge_representation.py:200-204).
#include "ktup_kg_pair.h"

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
  int serial;                    // option `deterministic`: one lane group of one workgroup walks every example (PairWalk)
};

template <int GL>
__global__ __launch_bounds__(256) void transd_step_kernel(TdStepArgs a) {
  const int lane = threadIdx.x % GL;
  const bool on = lane < a.nch;
  float part[4] = {0.f, 0.f, 0.f, 0.f};       // slot 1 (orthogonalLoss) stays 0 and is never written
  const float g1 = a.gscale;
  const bool track = a.gnorm != nullptr;
  const int gset = track ? gnorm_set(a.gnorm) : 0;
  float ssq = 0.f;
  const PairWalk<GL> walk(a.serial, a.B);
  for (int64_t k = walk.k0; k < a.B; k += walk.step) {
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
    if (a.regs & 2) norm_loss_rows<GL>(e, g1, lane, part[2], ge, he);
    if (a.regs & 4) norm_loss_rows<GL>(rr, g1, lane, part[3], gr, hr);
    auto scatter = [&](auto add) {    // a row that receives nothing gets no atomic
      RowAdded oe[4], oep[4], orr[2], orp[2];
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        oe[x] = add(a.gE + id[x] * a.lde + 4 * lane, ge[x], he[x]);
        oep[x] = add(a.gEp + id[x] * a.ldep + 4 * lane, gep[x], act);
      }
#pragma unroll
      for (int x = 0; x < 2; ++x) {
        orr[x] = add(a.gR + rid[x] * a.ldr + 4 * lane, gr[x], hr[x]);
        orp[x] = add(a.gRp + rid[x] * a.ldrp + 4 * lane, grp[x], act);
      }
      if (add.track) {
#pragma unroll
        for (int x = 0; x < 4; ++x) ssq += gain(oe[x]) + gain(oep[x]);
#pragma unroll
        for (int x = 0; x < 2; ++x) ssq += gain(orr[x]) + gain(orp[x]);
      }
    };
    if (on && track) scatter(RowAdd<true>{});
    else if (on) scatter(RowAdd<false>{});
  }
  step_tail(part, ssq, a.gnorm, gset, a.loss);
}

int launch_transd(const TdStepArgs& a, hipStream_t st, const char* name) {
  return with_lane_group(a.nch, [&](auto gl) {
    constexpr int GPB = 256 / decltype(gl)::value;
    const int grid = a.serial ? 1 : grid_for((a.B + GPB - 1) / GPB, 1024);
    hipLaunchKernelGGL((transd_step_kernel<decltype(gl)::value>), dim3(grid), dim3(256), 0, st, a);
    return check_launch(name);
  });
}

}  // namespace

#define KTUP_TDS_NONNULL(p) KTUP_REQUIRE((p) != nullptr, "%s: null pointer argument '" #p "'", name)

extern "C" int ktup_train_transd_step_supported(int d) { return lane_group_rows_ok(d, {}, {}); }

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
  if (!lane_group_rows_ok(d, {lde, ldr, ldep, ldrp}, {E, R, Ep, Rp, gE, gR, gEp, gRp}))
    return set_error(KTUP_ERR_UNSUPPORTED, "%s: needs d %% 4 == 0 (<= 256; got %d) and 16-byte aligned tables and gradients with pitches that are "
                     "multiples of 4 floats (see ktup_train_transd_step_supported)", name, d);
  TdStepArgs a{E, R, Ep, Rp, lde, ldr, ldep, ldrp, h, t, r, B, d / 4, l1 != 0, margin, gscale, regs, loss, gE, gR, gEp, gRp, gnorm,
               opt_deterministic() != 0};
  return launch_transd(a, (hipStream_t)stream, name);
}
