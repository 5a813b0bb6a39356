// The TransR training step in ONE launch (transR.py:65-78 + utils/misc.py:21-26 + knowledge_representation.py:176-204): both scores
// of every (positive, corrupted) pair, marginLoss, normLoss of the entity and relation rows and every gradient -- what the driver
// issued as a memset, three bucket launches, the bucketed forward, the margin loss, the bucketed backward and two regulariser
// launches (ktup_score_transr_mc.hip, ktup_loss.hip).  Those kernels are built for 307,200 triples: 1024-triple passes over a
// counting sort kept in caller scratch that a memset clears.  A 2 x 512-triple step needs none of it:
//   * workgroup (relation, split) reads the split's share of the relation ids and compacts the examples of ITS relation into LDS
//     (ballot + one LDS atomic per wave) -- no scratch, no memset, no second kernel, so the launch replays from a graph;
//   * M_r is staged in LDS once; a wave tile is 8 examples = 16 triples (column j < 8: the positive triple, column j + 8 its
//     corrupted twin), so both scores of an example sit in one wave and the hinge is decided by one lane exchange;
//   * the body is the bucketed backward's: y^T = M_r q^T + r and gq^T = M_r^T gy^T on v_mfma_f32_16x16x4_f32, gy (x) q accumulated
//     in registers over all tiles of the workgroup, one flush of non-zero cells per workgroup;
//   * an example whose twin names another relation (the reference's samplers never draw one, utils/data.py:23-56) goes to the
//     workgroup of its positive relation, which scores it one wave per example with both matrices streamed from L2.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ktup_common.h"
#include "ktup_lane_swap.h"

namespace ktup {
namespace {

constexpr int MAXB = 4096;   // examples per step (ids are kept as uint16 in LDS)
constexpr int PT = 8;        // examples per wave tile (16 triples)

template <int NCH_>
struct SGeom {
  static constexpr int NCH = NCH_, D = 4 * NCH;
  static constexpr int KG = (D + 15) / 16, CT = KG;
  static constexpr bool TAIL1 = NCH - 4 * (KG - 1) == 1;
  static constexpr int KGF = TAIL1 ? KG - 1 : KG;
  static constexpr int J = (16 * NCH + 63) / 64;
  static constexpr int TOTAL = 16 * NCH;
  static constexpr int PITCH4 = 4 * KG + 1, PITCHF = 4 * PITCH4;      // staged M_r rows (odd float4 pitch)
  static constexpr int M_F4 = 16 * CT * PITCH4;
  static constexpr int GYP = (16 * CT) % 32 == 16 ? 16 * CT : 16 * CT + 16;   // float pitch of the q / gy tiles: 16 (mod 32)
  static constexpr int XP4 = GYP / 4;
  static constexpr size_t TILE_BYTES = (size_t)16 * GYP * 4;
  static constexpr size_t WAVE_BYTES = 2 * TILE_BYTES + 64 * 4;      // q tile, gy tile, ids (head, tail) + slot flags
  static constexpr size_t FIXED = (size_t)M_F4 * 16 + (size_t)4 * CT * 16;
  static constexpr size_t TAIL_BYTES = (size_t)MAXB * 2 + 256;       // example list, counters, loss partials
  static constexpr int NW = FIXED + CT * WAVE_BYTES + TAIL_BYTES <= 160 * 1024 ? CT : (CT + 1) / 2;
  static constexpr int S = (CT + NW - 1) / NW;                        // output row tiles of gM per wave
  static constexpr size_t LDS = FIXED + NW * WAVE_BYTES + TAIL_BYTES;
};

struct TArgs {
  const v4* E; uint32_t lde4;
  const float* R; int64_t ldr;
  const float* M; int64_t ldm;
  const int64_t *h, *t, *r;     // [pos ; neg] rows: k and k + B
  int B, nsplit, l1, regs;      // regs: bit 1 normLoss(entity rows), bit 2 normLoss(relation rows)
  float margin, gscale;
  float* loss;                  // [4]: margin sum, -, normE, normR  (accumulated)
  float *gE, *gR, *gM;
};

template <typename G>
__global__ __launch_bounds__(G::NW * 64) void transr_step_kernel(TArgs a) {
  constexpr int NW = G::NW, S = G::S, NT = NW * 64;
  constexpr int NCH = G::NCH, D = G::D, CT = G::CT, KGF = G::KGF, J = G::J, TOTAL = G::TOTAL, PITCH4 = G::PITCH4, PITCHF = G::PITCHF;
  constexpr int GYP = G::GYP, XP4 = G::XP4;
  constexpr bool TAIL1 = G::TAIL1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  v4* Ms = reinterpret_cast<v4*>(smem);                                   // [16 CT rows][PITCH4]
  const float* Msf = reinterpret_cast<const float*>(Ms);
  v4* rS = Ms + G::M_F4;                                                  // [4 CT] relation vector, zero padded
  const float* rSf = reinterpret_cast<const float*>(rS);
  const int tid = threadIdx.x, lane = tid & 63, kq = lane >> 4, j = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  char* tiles = reinterpret_cast<char*>(rS + 4 * CT);
  auto qtile = [&](int ww) { return reinterpret_cast<v4*>(tiles + (size_t)ww * G::WAVE_BYTES); };
  auto gtile = [&](int ww) { return reinterpret_cast<v4*>(tiles + (size_t)ww * G::WAVE_BYTES + G::TILE_BYTES); };
  v4* xt = qtile(w);                                                      // [16 triples][XP4] q = h - t, zero beyond d
  v4* gyt = gtile(w);                                                     // [16 triples][XP4] gy
  int32_t* sid = reinterpret_cast<int32_t*>(tiles + (size_t)w * G::WAVE_BYTES + 2 * G::TILE_BYTES);   // [16] head, [16] tail, [16] slot in use
  uint16_t* list = reinterpret_cast<uint16_t*>(tiles + (size_t)NW * G::WAVE_BYTES);   // [MAXB]: this relation's examples from the front, strays from the back
  int32_t* cnts = reinterpret_cast<int32_t*>(list + MAXB);                // [2] (+ 2 pad)
  float* red = reinterpret_cast<float*>(cnts + 4);                        // [NW][4] loss partials
  const int rel = blockIdx.x / a.nsplit, sp = blockIdx.x - rel * a.nsplit;
  const int k_lo = (int)((int64_t)a.B * sp / a.nsplit), k_hi = (int)((int64_t)a.B * (sp + 1) / a.nsplit);
  const int64_t lde = (int64_t)a.lde4 * 4;
  const float* Ef = reinterpret_cast<const float*>(a.E);
  const bool l1 = a.l1 != 0;

  // ---- the examples of this (relation, split): positive relation == rel; the twin's relation decides between the tile path and the stray path
  if (tid < 2) cnts[tid] = 0;
  __syncthreads();
  for (int k0 = k_lo; k0 < k_hi; k0 += NT) {
    const int k = k0 + tid;
    bool mine = false, stray = false;
    if (k < k_hi && a.r[k] == (int64_t)rel) {
      mine = a.r[k + a.B] == (int64_t)rel;
      stray = !mine;
    }
    const uint64_t mm = __builtin_amdgcn_ballot_w64(mine), ms = __builtin_amdgcn_ballot_w64(stray);
    int bm = 0, bs = 0;
    if (lane == 0) {
      if (mm) bm = atomicAdd(&cnts[0], __popcll(mm));
      if (ms) bs = atomicAdd(&cnts[1], __popcll(ms));
    }
    bm = __shfl(bm, 0, 64);
    bs = __shfl(bs, 0, 64);
    const uint64_t below = (1ull << lane) - 1ull;
    if (mine) list[bm + __popcll(mm & below)] = (uint16_t)k;
    if (stray) list[MAXB - 1 - (bs + __popcll(ms & below))] = (uint16_t)k;
  }
  __syncthreads();
  const int cnt = cnts[0], nstray = cnts[1];
  if (cnt + nstray == 0) return;                                          // (workgroup uniform)

  if (cnt > 0) {                                                          // stage M_r (rows >= d and columns >= d are zero) and r
    const float* Mg = a.M + (int64_t)rel * a.ldm;
    float* Mw = reinterpret_cast<float*>(Ms);
    for (int idx = tid; idx < G::M_F4 * 4; idx += NT) {
      const int row = idx / PITCHF, k = idx - row * PITCHF;
      Mw[idx] = (row < D && k < D) ? Mg[row * D + k] : 0.f;
    }
    float* rw = reinterpret_cast<float*>(rS);
    for (int idx = tid; idx < 16 * CT; idx += NT) rw[idx] = idx < D ? a.R[(int64_t)rel * a.ldr + idx] : 0.f;
  }
  for (int idx = lane; idx < 2 * 16 * XP4; idx += 64) xt[idx] = (v4){0.f, 0.f, 0.f, 0.f};   // both tiles: finite from the start

  float part0 = 0.f, part2 = 0.f, part3 = 0.f;                            // marginLoss, normLoss(entity rows), normLoss(relation rows)
  const float g1 = a.gscale;

  // ---- normLoss of the 4 entity rows of every example of this workgroup, strays included (utils/loss.py:21-23): a 32-lane group per row
  if (a.regs & 2) {
    const int gl = tid & 31;
    const bool on = gl < NCH;
    const int total = 4 * (cnt + nstray);
    for (int item = tid >> 5; item < total; item += 2 * NW) {
      const int p = item >> 2, x = item & 3;                              // x: ph, pt, nh, nt
      const int k = p < cnt ? list[p] : list[MAXB - 1 - (p - cnt)];
      const int64_t at = (int64_t)k + ((x >> 1) ? a.B : 0);
      const int64_t id = (x & 1) ? a.t[at] : a.h[at];
      const v4 e = on ? a.E[(uint64_t)id * a.lde4 + (uint32_t)gl] : (v4){0.f, 0.f, 0.f, 0.f};
      const float s = group_sum<32>(fmaf(e[0], e[0], fmaf(e[1], e[1], fmaf(e[2], e[2], e[3] * e[3]))));
      if (s - 1.f > 0.f) {
        if (on) {
          float* dst = a.gE + id * lde + 4 * gl;
          const float c = 2.f * g1;
#pragma unroll
          for (int c4 = 0; c4 < 4; ++c4) atomicAdd(dst + c4, c * e[c4]);
        }
        if (gl == 0) part2 += s - 1.f;
      }
    }
  }
  __syncthreads();                                                        // M_r, r and the zeroed tiles are in place

  // ---- the tile path
  int grow[J], gc[J];
#pragma unroll
  for (int jj = 0; jj < J; ++jj) {
    const int e = lane + 64 * jj;
    const bool past = e >= TOTAL;
    grow[jj] = past ? 0 : e / NCH;
    gc[jj] = past ? 0 : e % NCH;
  }
  const bool last_ok = lane + 64 * (J - 1) < TOTAL;
  const v4* xb = xt + j * XP4 + kq;
  const v4* mrow = Ms + j * PITCH4 + kq;
  v4 accM[S][CT], accR[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    accR[s] = (v4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int cb = 0; cb < CT; ++cb) accM[s][cb] = (v4){0.f, 0.f, 0.f, 0.f};
  }
  const float one0 = j == 0 ? 1.f : 0.f;
  for (int sub0 = 0; sub0 * PT < cnt; sub0 += NW) {
    const int sub = sub0 + w;
    const bool valid = sub * PT < cnt;                                    // wave uniform
    if (valid) {
      if (lane < 16) {
        const int p = lane & 7;
        const bool on = sub * PT + p < cnt;
        const int k = list[on ? sub * PT + p : sub * PT];                 // unused slots re-read the tile's first example, with g = 0
        const int64_t at = (int64_t)k + ((lane >> 3) ? a.B : 0);
        sid[lane] = (int32_t)a.h[at];
        sid[16 + lane] = (int32_t)a.t[at];
        sid[32 + lane] = on ? 1 : 0;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      {                                                                   // q = h - t -> LDS tile
        v4 hh[J], tt[J];
#pragma unroll
        for (int jj = 0; jj < J; ++jj) {
          asm volatile("" : "+v"(gc[jj]));
          const uint32_t ih = (uint32_t)sid[grow[jj]], it = (uint32_t)sid[16 + grow[jj]];
          hh[jj] = a.E[(uint64_t)ih * a.lde4 + (uint32_t)gc[jj]];
          tt[jj] = a.E[(uint64_t)it * a.lde4 + (uint32_t)gc[jj]];
        }
#pragma unroll
        for (int jj = 0; jj < J; ++jj) {
          if (jj < J - 1 || last_ok) xt[grow[jj] * XP4 + gc[jj]] = hh[jj] + (-tt[jj]);
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      // ---- phase 1: y^T tiles (lane (kq, j): coordinates 16 ct + 4 kq + reg of triple j), both scores, the hinge, gy^T in the same registers
      v4 bq[KGF];
#pragma unroll
      for (int g = 0; g < KGF; ++g) bq[g] = xb[4 * g];                    // chunks beyond d are zero in the tile
      float btail = 0.f;
      if (TAIL1) btail = reinterpret_cast<const float*>(xt + j * XP4 + 4 * KGF)[kq];
      v4 gy[CT];
      v4 dacc = (v4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        v4 acc = rS[4 * ct + kq];
#pragma unroll
        for (int g = 0; g < KGF; ++g) {
          const v4 av = mrow[ct * 16 * PITCH4 + 4 * g];
#pragma unroll
          for (int c = 0; c < 4; ++c) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[c], bq[g][c], acc, 0, 0, 0);
        }
        if (TAIL1) {
          const float as = reinterpret_cast<const float*>(Ms + (ct * 16 + j) * PITCH4 + 4 * KGF)[kq];
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(as, btail, acc, 0, 0, 0);
        }
        // rows >= d of M and entries >= d of r are zero, so padded coordinates contribute dist(0) = 0
        if (l1) dacc += __builtin_elementwise_abs(acc);
        else dacc = __builtin_elementwise_fma(acc, acc, dacc);
        gy[ct] = acc;
      }
      const float sc = allsum_kq((dacc[0] + dacc[1]) + (dacc[2] + dacc[3]));   // score of triple j, in its four kq lanes
      const float other = __shfl_xor(sc, 8, 64);                          // the twin's
      const bool negcol = j >= 8;
      const float arg = (negcol ? other - sc : sc - other) + a.margin;    // pos - neg + margin (utils/loss.py:8-16)
      const bool act = sid[32 + j] != 0 && arg > 0.f;
      if (lane < 8 && act) part0 += arg;
      const float gj = act ? (negcol ? -g1 : g1) : 0.f;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
#pragma unroll
        for (int c = 0; c < 4; ++c) gy[ct][c] = gj * ddist1(gy[ct][c], l1);   // padded coordinates: y = 0 -> 0
        gyt[j * XP4 + 4 * ct + kq] = gy[ct];
      }
      // ---- phase 2: gq^T = M^T gy^T; A = M[16 ct + 4 kq + reg][16 ct2 + j] (a column walk of the staged rows)
      const int64_t hj = sid[j], tj = sid[16 + j];
      if (__builtin_amdgcn_ballot_w64(gj != 0.f)) {                       // (a tile without an active example adds nothing)
#pragma unroll
        for (int ct2 = 0; ct2 < CT; ++ct2) {
          v4 gq = (v4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
              const float am = Msf[(16 * ct + 4 * kq + reg) * PITCHF + 16 * ct2 + j];
              gq = __builtin_amdgcn_mfma_f32_16x16x4f32(am, gy[ct][reg], gq, 0, 0, 0);
            }
          }
          const int c0 = 16 * ct2 + 4 * kq;
          if (gj != 0.f && hj != tj && c0 < D) {                          // (h == t: +gq and -gq on one row are exactly nothing)
            atomic_add4(a.gE + hj * lde + c0, make_float4(gq[0], gq[1], gq[2], gq[3]));
            atomic_add4(a.gE + tj * lde + c0, make_float4(-gq[0], -gq[1], -gq[2], -gq[3]));
          }
        }
      }
    } else {
      for (int idx = lane; idx < 16 * XP4; idx += 64) gyt[idx] = (v4){0.f, 0.f, 0.f, 0.f};   // nothing from this wave in this round
    }
    __syncthreads();
    // ---- phase 3: gM row tiles of this wave over the round's NW x 16 triples; ones column -> gR
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const int ca = w + s * NW;
      if (ca < CT) {
        for (int ww = 0; ww < NW; ++ww) {
          if ((sub0 + ww) * PT >= cnt) break;                             // later waves had no examples either
          const float* gf = reinterpret_cast<const float*>(gtile(ww));
          const float* qf = reinterpret_cast<const float*>(qtile(ww));
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) {
            const float av = gf[(4 * kk + kq) * GYP + 16 * ca + j];
            accR[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, one0, accR[s], 0, 0, 0);
#pragma unroll
            for (int cb = 0; cb < CT; ++cb) {
              const float bv = qf[(4 * kk + kq) * GYP + 16 * cb + j];
              accM[s][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, accM[s][cb], 0, 0, 0);
            }
          }
        }
      }
    }
    __syncthreads();                                                      // the next round (and the stray path) rewrites the tiles
  }
  if (cnt > 0) {
    // ---- one flush per workgroup: this wave's row tiles of gM[rel] and gR[rel]; cells that received nothing are not touched
    float* gm = a.gM + (int64_t)rel * a.ldm;
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const int ca = w + s * NW;
      if (ca < CT) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int i = 16 * ca + 4 * kq + reg;
          if (i < D) {
#pragma unroll
            for (int cb = 0; cb < CT; ++cb) {
              const int k = 16 * cb + j;
              const float v = accM[s][cb][reg];
              if (k < D && v != 0.f) atomicAdd(gm + (int64_t)i * D + k, v);
            }
            if (j == 0 && accR[s][reg] != 0.f) atomicAdd(a.gR + (int64_t)rel * a.ldr + i, accR[s][reg]);
          }
        }
      }
    }
    // ---- normLoss of the relation row: it occurs 2 cnt times (every occurrence counts, as in ktup_reg_norm_fused)
    if ((a.regs & 4) && w == 0) {
      float s = 0.f;
      for (int i = lane; i < 16 * CT; i += 64) s = fmaf(rSf[i], rSf[i], s);
      s = group_sum<64>(s);
      if (s - 1.f > 0.f) {
        const float occ = 2.f * (float)cnt;
        const float c = 2.f * g1 * occ;
        for (int i = lane; i < D; i += 64) atomicAdd(a.gR + (int64_t)rel * a.ldr + i, c * rSf[i]);
        if (lane == 0) part3 += occ * (s - 1.f);
      }
    }
  }

  // ---- the stray path: one wave per example, both matrices streamed from L2, the wave's two tiles as scratch
  {
    float* qs = reinterpret_cast<float*>(xt);                             // [2][D] q of the positive and the corrupted triple
    float* ys = reinterpret_cast<float*>(gyt);                            // [2][D] y, then gy
    for (int sx = w; sx < nstray; sx += NW) {
      const int k = list[MAXB - 1 - sx];
      int64_t hid[2], tl[2], rid[2];
      float scx[2];
#pragma unroll
      for (int x = 0; x < 2; ++x) {
        const int64_t at = (int64_t)k + (x ? a.B : 0);
        hid[x] = a.h[at]; tl[x] = a.t[at]; rid[x] = a.r[at];
        for (int c = lane; c < D; c += 64) qs[x * D + c] = Ef[hid[x] * lde + c] - Ef[tl[x] * lde + c];
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int x = 0; x < 2; ++x) {
        const float* Mg = a.M + rid[x] * a.ldm;
        float s = 0.f;
        for (int i = lane; i < D; i += 64) {
          float y = a.R[rid[x] * a.ldr + i];
          for (int c = 0; c < D; ++c) y = fmaf(Mg[i * D + c], qs[x * D + c], y);
          ys[x * D + i] = y;
          s += dist1(y, l1);
        }
        scx[x] = group_sum<64>(s);
      }
      const float arg = scx[0] - scx[1] + a.margin;
      const bool act = arg > 0.f;
      if (lane == 0 && act) part0 += arg;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int x = 0; x < 2; ++x) {
        const float* Mg = a.M + rid[x] * a.ldm;
        if (act) {
          const float g = x ? -g1 : g1;
          for (int i = lane; i < D; i += 64) {
            const float v = g * ddist1(ys[x * D + i], l1);
            ys[x * D + i] = v;
            if (v != 0.f) atomicAdd(a.gR + rid[x] * a.ldr + i, v);
          }
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          for (int idx = lane; idx < D * D; idx += 64) {
            const int i = idx / D, c = idx - i * D;
            const float v = ys[x * D + i] * qs[x * D + c];
            if (v != 0.f) atomicAdd(a.gM + rid[x] * a.ldm + idx, v);
          }
          for (int c = lane; c < D; c += 64) {
            float gq = 0.f;
            for (int i = 0; i < D; ++i) gq = fmaf(Mg[i * D + c], ys[x * D + i], gq);
            if (hid[x] != tl[x]) {                                          // (h == t: +gq and -gq on one row are exactly nothing)
              atomicAdd(a.gE + hid[x] * lde + c, gq);
              atomicAdd(a.gE + tl[x] * lde + c, -gq);
            }
          }
        }
        if (a.regs & 4) {
          float s = 0.f;
          for (int i = lane; i < D; i += 64) { const float v = a.R[rid[x] * a.ldr + i]; s = fmaf(v, v, s); }
          s = group_sum<64>(s);
          if (s - 1.f > 0.f) {
            for (int i = lane; i < D; i += 64) atomicAdd(a.gR + rid[x] * a.ldr + i, 2.f * g1 * a.R[rid[x] * a.ldr + i]);
            if (lane == 0) part3 += s - 1.f;
          }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  }

  // ---- the loss slots: wave sums -> one atomic per workgroup and slot
  part0 = group_sum<64>(part0); part2 = group_sum<64>(part2); part3 = group_sum<64>(part3);
  if (lane == 0) { red[4 * w + 0] = part0; red[4 * w + 1] = 0.f; red[4 * w + 2] = part2; red[4 * w + 3] = part3; }
  __syncthreads();
  if (tid < 4 && tid != 1) {
    float v = 0.f;
    for (int ww = 0; ww < NW; ++ww) v += red[4 * ww + tid];
    if (v != 0.f) atomicAdd(a.loss + tid, v);
  }
}

template <typename G>
int launch_step(TArgs a, int64_t n_rel, int nsplit, hipStream_t st, const char* name) {
  static_assert(G::LDS <= 160 * 1024, "LDS budget");
  static_assert(G::NW <= 8, "loss partials: 8 waves");
  if (nsplit == 0) {   // one round of the workgroup's waves for a relation's expected share of the batch
    const int64_t share = (a.B + n_rel - 1) / n_rel;
    nsplit = (int)((share + G::NW * PT - 1) / (G::NW * PT));
  }
  a.nsplit = nsplit < 1 ? 1 : nsplit > 32 ? 32 : nsplit;
  if (a.nsplit > a.B) a.nsplit = a.B;
  (void)hipFuncSetAttribute((const void*)transr_step_kernel<G>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)G::LDS);
  hipLaunchKernelGGL((transr_step_kernel<G>), dim3((unsigned)(n_rel * a.nsplit)), dim3(G::NW * 64), G::LDS, st, a);
  return check_launch(name);
}

}  // namespace
}  // namespace ktup

using namespace ktup;

extern "C" int ktup_train_transr_step_supported(int d) { return (d == 64 || d == 100 || d == 128) && !opt_deterministic(); }

extern "C" int ktup_train_transr_step(const float* E, int64_t lde, const float* R, int64_t ldr, const float* M, int64_t ldm, int64_t n_rel,
                                      int d, const int64_t* h, const int64_t* t, const int64_t* r, int64_t B, int l1, float margin,
                                      float gscale, int regs, int nsplit, float* loss, float* gE, float* gR, float* gM, void* stream) {
  const char* name = "ktup_train_transr_step";
  KTUP_REQUIRE(B >= 0 && n_rel >= 0 && nsplit >= 0, "%s: negative sizes", name);
  KTUP_REQUIRE(E && R && M && h && t && r && loss && gE && gR && gM, "%s: null pointer argument", name);
  KTUP_REQUIRE((regs & ~6) == 0, "%s: regs takes bit 1 (normLoss of the entity rows) and bit 2 (normLoss of the relation rows); TransR has no "
               "orthogonalLoss (bit 0)", name);
  if (opt_deterministic())
    return set_error(KTUP_ERR_UNSUPPORTED, "%s: the gradients are float atomics of many workgroups (option deterministic is set)", name);
  if (d != 64 && d != 100 && d != 128) return set_error(KTUP_ERR_UNSUPPORTED, "%s: d=%d (takes 64, 100, 128; see ktup_train_transr_step_supported)", name, d);
  if (B < 1 || B > MAXB || n_rel < 1 || n_rel > 4096)
    return set_error(KTUP_ERR_UNSUPPORTED, "%s: takes 1 <= B <= %d and 1 <= n_rel <= 4096 (B=%lld, n_rel=%lld)", name, MAXB, (long long)B, (long long)n_rel);
  if (((lde | ldr | ldm) & 3) || lde < d || ldr < d || ldm < (int64_t)d * d || (lde >> 2) > 0xffffffffll || !aligned16(E) || !aligned16(R) ||
      !aligned16(M) || !aligned16(gE) || !aligned16(gR) || !aligned16(gM))
    return set_error(KTUP_ERR_UNSUPPORTED, "%s: needs 16-byte aligned tables and gradients with pitches that are multiples of 4 floats", name);
  TArgs a{reinterpret_cast<const v4*>(E), (uint32_t)(lde >> 2), R, ldr, M, ldm, h, t, r, (int)B, 0, l1, regs, margin, gscale, loss, gE, gR, gM};
  hipStream_t st = (hipStream_t)stream;
  if (d == 64) return launch_step<SGeom<16>>(a, n_rel, nsplit, st, name);
  if (d == 100) return launch_step<SGeom<25>>(a, n_rel, nsplit, st, name);
  return launch_step<SGeom<32>>(a, n_rel, nsplit, st, name);
}
