// TransD: fused gather + score and its backward (transD.py:61-76, utils/misc.py:36-37).
//
//   h_perp = h + (h . h_p) r_p,   t_perp = t + (t . t_p) r_p,   v = h_perp + r - t_perp = (h - t) + r + (alpha - beta) r_p
// with alpha = h . h_p, beta = t . t_p.  Six rows per triple (h, t, h_p, t_p, r, r_p).  G = 16 / 32 / 64 consecutive lanes own one
// triple and walk its rows in 16-byte (or, for unaligned tables / d % 4 != 0, 4-byte) pieces, any d: nothing is kept per coordinate,
// the passes re-read the rows (they sit in L1 / L2 after the first pass).  The B = 512 step is bound by its launches, not by this.
// Backward, with g = gscore * dist'(v) and gamma = g . r_p:
//   dh = g + gamma h_p    dh_p = gamma h    dt = -g - gamma t_p    dt_p = -gamma t    dr = g    dr_p = (alpha - beta) g
// added into the caller's buffers with float atomics.
#include "ktup_rows.h"

using namespace ktup;

namespace {

struct TdArgs {
  const float *E, *R, *Ep, *Rp;
  int64_t lde, ldr, ldep, ldrp;
  const int64_t *h, *t, *r;
  bool l1;
  float* score;          // forward
  const float* gs;       // backward
  float *gE, *gR, *gEp, *gRp;
};

template <typename V, int G>
__global__ __launch_bounds__(256) void transd_fwd_kernel(TdArgs a, int nch, int64_t n) {
  const int lane = threadIdx.x % G;
  constexpr int GPB = 256 / G;
  for (int64_t row = (int64_t)blockIdx.x * GPB + threadIdx.x / G; row < n; row += (int64_t)gridDim.x * GPB) {
    const int64_t hr = a.h[row], tr = a.t[row], rr = a.r[row];
    const V* ph = reinterpret_cast<const V*>(a.E + hr * a.lde);
    const V* pt = reinterpret_cast<const V*>(a.E + tr * a.lde);
    const V* php = reinterpret_cast<const V*>(a.Ep + hr * a.ldep);
    const V* ptp = reinterpret_cast<const V*>(a.Ep + tr * a.ldep);
    const V* pr = reinterpret_cast<const V*>(a.R + rr * a.ldr);
    const V* prp = reinterpret_cast<const V*>(a.Rp + rr * a.ldrp);
    float al = 0.f, be = 0.f;
    for (int c = lane; c < nch; c += G) { al += vdot(ph[c], php[c]); be += vdot(pt[c], ptp[c]); }
    al = group_sum<G>(al);
    be = group_sum<G>(be);
    float s = 0.f;
    for (int c = lane; c < nch; c += G) {
      const V rp = prp[c];
      const V hp = vfma(al, rp, ph[c]), tp = vfma(be, rp, pt[c]);     // the reference's order: e + (e . e_p) r_p, then h + r - t
      s += vdist(vsub(vadd(hp, pr[c]), tp), a.l1);
    }
    s = group_sum<G>(s);
    if (lane == 0) a.score[row] = s;
  }
}

template <typename V, int G>
__global__ __launch_bounds__(256) void transd_bwd_kernel(TdArgs a, int nch, int64_t n) {
  const int lane = threadIdx.x % G;
  constexpr int GPB = 256 / G, W = VW<V>::W;
  for (int64_t row = (int64_t)blockIdx.x * GPB + threadIdx.x / G; row < n; row += (int64_t)gridDim.x * GPB) {
    const int64_t hr = a.h[row], tr = a.t[row], rr = a.r[row];
    const V* ph = reinterpret_cast<const V*>(a.E + hr * a.lde);
    const V* pt = reinterpret_cast<const V*>(a.E + tr * a.lde);
    const V* php = reinterpret_cast<const V*>(a.Ep + hr * a.ldep);
    const V* ptp = reinterpret_cast<const V*>(a.Ep + tr * a.ldep);
    const V* pr = reinterpret_cast<const V*>(a.R + rr * a.ldr);
    const V* prp = reinterpret_cast<const V*>(a.Rp + rr * a.ldrp);
    const float gsc = a.gs[row];
    float al = 0.f, be = 0.f;
    for (int c = lane; c < nch; c += G) { al += vdot(ph[c], php[c]); be += vdot(pt[c], ptp[c]); }
    al = group_sum<G>(al);
    be = group_sum<G>(be);
    float gam = 0.f;
    for (int c = lane; c < nch; c += G) {
      const V rp = prp[c];
      const V hp = vfma(al, rp, ph[c]), tp = vfma(be, rp, pt[c]);
      gam += vdot(vscale(gsc, vddist(vsub(vadd(hp, pr[c]), tp), a.l1)), rp);
    }
    gam = group_sum<G>(gam);
    const float ab = al - be;
    for (int c = lane; c < nch; c += G) {
      const V rp = prp[c], hv = ph[c], tv = pt[c];
      const V hp = vfma(al, rp, hv), tp = vfma(be, rp, tv);
      const V g = vscale(gsc, vddist(vsub(vadd(hp, pr[c]), tp), a.l1));
      const int64_t o = (int64_t)c * W;
      vatomic(a.gE + hr * a.lde + o, vfma(gam, php[c], g));
      vatomic(a.gEp + hr * a.ldep + o, vscale(gam, hv));
      vatomic(a.gE + tr * a.lde + o, vscale(-1.f, vfma(gam, ptp[c], g)));
      vatomic(a.gEp + tr * a.ldep + o, vscale(-gam, tv));
      vatomic(a.gR + rr * a.ldr + o, g);
      vatomic(a.gRp + rr * a.ldrp + o, vscale(ab, g));
    }
  }
}

template <bool BWD>
int launch(const TdArgs& a, int d, bool vec4, int64_t n, hipStream_t st, const char* name) {
  const int nch = vec4 ? d / 4 : d;
#define KTUP_TD(V, G)                                                                                   \
  {                                                                                                     \
    const int grid = grid_for((n + (256 / G) - 1) / (256 / G));                                         \
    if (BWD) hipLaunchKernelGGL((transd_bwd_kernel<V, G>), dim3(grid), dim3(256), 0, st, a, nch, n);    \
    else hipLaunchKernelGGL((transd_fwd_kernel<V, G>), dim3(grid), dim3(256), 0, st, a, nch, n);        \
    return check_launch(name);                                                                          \
  }
  if (vec4) {
    if (nch <= 16) KTUP_TD(float4, 16)
    if (nch <= 32) KTUP_TD(float4, 32)
    KTUP_TD(float4, 64)
  }
  if (nch <= 16) KTUP_TD(float, 16)
  if (nch <= 32) KTUP_TD(float, 32)
  KTUP_TD(float, 64)
#undef KTUP_TD
}

}  // namespace

#define KTUP_TD_NONNULL(p) KTUP_REQUIRE((p) != nullptr, "%s: null pointer argument '" #p "'", name)

extern "C" int ktup_score_transd_fwd(const float* E, int64_t lde, const float* R, int64_t ldr, const float* Ep, int64_t ldep,
                                     const float* Rp, int64_t ldrp, int d, const int64_t* h, const int64_t* t, const int64_t* r,
                                     int64_t n, int l1, float* score, void* stream) {
  const char* name = "ktup_score_transd_fwd";
  KTUP_REQUIRE(d > 0, "%s: embedding_size must be positive (got %d)", name, d);
  KTUP_REQUIRE(n >= 0, "%s: negative batch size", name);
  if (n == 0) return KTUP_OK;
  KTUP_TD_NONNULL(E); KTUP_TD_NONNULL(R); KTUP_TD_NONNULL(Ep); KTUP_TD_NONNULL(Rp);
  KTUP_TD_NONNULL(h); KTUP_TD_NONNULL(t); KTUP_TD_NONNULL(r); KTUP_TD_NONNULL(score);
  TdArgs a{E, R, Ep, Rp, lde, ldr, ldep, ldrp, h, t, r, l1 != 0, score, nullptr, nullptr, nullptr, nullptr, nullptr};
  return launch<false>(a, d, can_vec4(d, {E, R, Ep, Rp}, {lde, ldr, ldep, ldrp}), n, (hipStream_t)stream, name);
}

extern "C" int ktup_score_transd_bwd(const float* E, int64_t lde, const float* R, int64_t ldr, const float* Ep, int64_t ldep,
                                     const float* Rp, int64_t ldrp, int d, const int64_t* h, const int64_t* t, const int64_t* r,
                                     int64_t n, int l1, const float* gscore, float* gE, float* gR, float* gEp, float* gRp,
                                     void* stream) {
  const char* name = "ktup_score_transd_bwd";
  KTUP_REQUIRE(d > 0, "%s: embedding_size must be positive (got %d)", name, d);
  KTUP_REQUIRE(n >= 0, "%s: negative batch size", name);
  if (n == 0) return KTUP_OK;
  KTUP_TD_NONNULL(E); KTUP_TD_NONNULL(R); KTUP_TD_NONNULL(Ep); KTUP_TD_NONNULL(Rp);
  KTUP_TD_NONNULL(h); KTUP_TD_NONNULL(t); KTUP_TD_NONNULL(r); KTUP_TD_NONNULL(gscore);
  KTUP_TD_NONNULL(gE); KTUP_TD_NONNULL(gR); KTUP_TD_NONNULL(gEp); KTUP_TD_NONNULL(gRp);
  TdArgs a{E, R, Ep, Rp, lde, ldr, ldep, ldrp, h, t, r, l1 != 0, nullptr, gscore, gE, gR, gEp, gRp};
  return launch<true>(a, d, can_vec4(d, {E, R, Ep, Rp, gE, gR, gEp, gRp}, {lde, ldr, ldep, ldrp}), n, (hipStream_t)stream, name);
}
