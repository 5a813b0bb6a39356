// The score code of the preference-space evaluation passes (soft gate, squared L2), ONCE: the geometry of the operand tables (QGeom),
// a lane's A operands of the whole pass, the LDS-DMA of a 16-item tile, the MFMA chain of a 16 x 16 tile and the four-term epilogue.
// ktup_eval_pass.hip (the list pass eval_pass_q_kernel: the filtered top-n of every user) and ktup_pref_rank_pass.hip (the rank pass:
// the filtered rank of every gold item) include it, so a (user, item) score is the same bits in both; the formulation, the history
// and the measurements are in ktup_eval_pass.hip's comments.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ktup_common.h"
#include "ktup_lane_swap.h"

namespace ktup {
namespace {

constexpr int IBT = 16;        // items per LDS tile

// Six d-long products per pair (u.NV, NU.v, AU.C0, AU.NV, NU.C0, NU.NV: round 2's first fused pass, 0.39 ms per ml1m sweep) are
// more work than the model needs.  With the soft gate every vector of the score lives in
//   span{x} + span{Ar_p} + span{Cn_p}   (x = u or v;  RU = sum_p L_p Ar_p,  NU = sum_p L_p Cn_p,  L = Alog x, P <= 32 preferences)
// so every user x item cross term except u.v is a P-long contraction of per-row P-vectors (L, Rx = Ar x, Nx = Cn x) through the
// three P x P Gram matrices G_RR = Ar Ar^T, G_RN = Ar Cn^T, G_NN = Cn Cn^T:
//   s  cross = u.NV - v.NU            = [ Nu ; -L ]                          . [ LV ; Nv ]          K = 2 P
//   an cross = AU.NV - C0.NU          = [ Nu + G_RN^T L + G_RN L ; -L ]      . [ LV ; Nv ]          K = 2 P   (same B)
//   nn cross = 2 NU.NV                = [ 2 G_NN L ]                         . [ LV ]               K = P     (same B)
//   aa cross = -2 AU.C0               = [ -2u ; -2L ; 2 (Ru + G_RR L) ]      . [ v ; Rv ; LV ]      K = d + 2 P
// with the Gram products folded into the USER operand once per pass.  At d = 100, P = 20: 68 MFMAs (K padded to 16-blocks) and
// 12 ds_read_b128 per 16 x 16 tile instead of 156 and 75; an item row is 160 floats instead of 300.  Scores agree with the
// d-space kernels to fp32 rounding (a different association of the same sums), not bit for bit.
template <int NCH_, int NP_>
struct QGeom {
  static constexpr int NCH = NCH_, D = 4 * NCH, NP = NP_, P4 = 4 * NP;
  static constexpr int ROWB = D + 3 * P4;                       // item row: [x ; Rx ; L ; Nx]
  static constexpr int RB4 = ROWB / 4;
  // An item row is [x ; Rx ; L ; Nx | its 4 scalars (| one zero float4)] at an ODD float4 pitch (16 rows x 4 k-quads tile the LDS banks)
  // -- in memory exactly as in LDS, so a tile of 16 consecutive items is ONE contiguous run of IBT * ROW4 float4 and travels by
  // LDS-DMA (global_load_lds_dwordx4: destination = a wave-uniform LDS address + 16 B x lane): no staging registers (they were 12 of
  // the lane's 168, with 9 more for the lane-constant source / destination addresses: 18 spilled), no ds_write pass (whose 16-lane
  // groups straddled the row pads: ~16 two-way bank conflicts per tile)
  static constexpr int ROW4 = (RB4 + 1) | 1;
  static constexpr int GROW = 4 * ROW4;                         // floats per item row
  static constexpr int TSLOTS = IBT * ROW4;                     // float4 per tile
  static constexpr int DPW = ((TSLOTS + 63) / 64 + 3) / 4;      // DMA instructions per wave and tile (wave w issues pieces w, w + 4, ...)
  static constexpr int SOFF4 = (D + P4) / 4;                    // float4 offset of [L ; Nx] inside a row
  static constexpr int KA = (D + 2 * P4 + 15) / 16, KS = (2 * P4 + 15) / 16, KN = (P4 + 15) / 16;   // 16-blocks of K
  static constexpr int NA = KA + 2 * KS + KN;                   // float4 per lane and 16-block of a user row in memory: [AA | S | AN | NN]
  static constexpr int AROW = 16 * NA;                          // floats per user row
  // What the sweep multiplies is the REAL K of each product: whole 16-blocks (one ds_read_b128 and four MFMAs each, k = 16 g + 4 kq + c)
  // and then the remaining k-quads one MFMA each (one ds_read_b32, k = 16 F + 4 m + kq) -- the zero padding of the last 16-blocks
  // was 8 of 68 MFMAs per tile at d = 100, P = 20
  static constexpr int FA = (D + 2 * P4) / 16, TA = ((D + 2 * P4) % 16) / 4;     // AA: [x ; Rx ; L]
  static constexpr int FS = (2 * P4) / 16, TS = ((2 * P4) % 16) / 4;             // S and AN: [L ; Nx]
  static constexpr int FN = P4 / 16, TN = (P4 % 16) / 4;                         // NN: [L]
  static constexpr int NREG = 4 * FA + TA + 2 * (4 * FS + TS) + 4 * FN + TN;     // A-operand registers per lane
  static constexpr int SUB = 1;                                 // 16-item sub-tiles per buffer = per workgroup barrier (2: no faster, and the
                                                                // pending-candidate buffers below need the LDS for three workgroups per CU)
  static constexpr int TILE_F4 = SUB * IBT * ROW4 + 4;          // + pad: the padded K blocks read a little past the last row
#ifndef KTUP_EVAL_MINW3
#define KTUP_EVAL_MINW3 3
#endif
  static constexpr int MINW = NREG <= 64 ? KTUP_EVAL_MINW3 : 2;                 // waves per SIMD the register budget allows (= workgroups per CU)
};

// The next three pieces are MACROS, not functions: as functions (force-inlined or not, the operands in a struct or in eight arrays)
// every instantiation of the list pass came out with another register allocation than it had before the move -- the inliner hands
// the optimiser the same operations in another order -- and the list pass is to stay the machine code it was
// (profiles/pref_ranks_narrow_check.txt).  Expanded text is the same text.  q_score below is a function: it inlines to the same code.
//
// KTUP_Q_USER_OPS(G, OK, ROW, KQ): declares a lane's A operands of the whole pass -- aAA, aS, aAN, aNN (k-quad KQ of every whole 16-block)
// and tAA, tS, tAN, tNN (element KQ of every remaining k-quad) -- and loads them from the user's operand row ROW (a const float*; the
// expression may use `ok`) where OK, zeros elsewhere.
#define KTUP_Q_USER_OPS(G, OK, ROW, KQ)                                                                                                   \
  v4 aAA[G::FA > 0 ? G::FA : 1], aS[G::FS > 0 ? G::FS : 1], aAN[G::FS > 0 ? G::FS : 1], aNN[G::FN > 0 ? G::FN : 1];                       \
  float tAA[G::TA > 0 ? G::TA : 1], tS[G::TS > 0 ? G::TS : 1], tAN[G::TS > 0 ? G::TS : 1], tNN[G::TN > 0 ? G::TN : 1];                    \
  {                                                                                                                                       \
    const bool ok = OK;                                                                                                                   \
    const float* rf = ROW;                                                                                                                \
    const v4* r0 = reinterpret_cast<const v4*>(rf);                                                                                       \
    constexpr int oS = 16 * G::KA, oAN = oS + 16 * G::KS, oNN = oAN + 16 * G::KS;                                                         \
    const v4 z4 = (v4){0.f, 0.f, 0.f, 0.f};                                                                                               \
    _Pragma("unroll") for (int g = 0; g < G::FA; ++g) aAA[g] = ok ? r0[4 * g + KQ] : z4;                                                  \
    _Pragma("unroll") for (int m = 0; m < G::TA; ++m) tAA[m] = ok ? rf[16 * G::FA + 4 * m + KQ] : 0.f;                                    \
    _Pragma("unroll") for (int g = 0; g < G::FS; ++g) {                                                                                   \
      aS[g] = ok ? r0[oS / 4 + 4 * g + KQ] : z4;                                                                                          \
      aAN[g] = ok ? r0[oAN / 4 + 4 * g + KQ] : z4;                                                                                        \
    }                                                                                                                                     \
    _Pragma("unroll") for (int m = 0; m < G::TS; ++m) {                                                                                   \
      tS[m] = ok ? rf[oS + 16 * G::FS + 4 * m + KQ] : 0.f;                                                                                \
      tAN[m] = ok ? rf[oAN + 16 * G::FS + 4 * m + KQ] : 0.f;                                                                              \
    }                                                                                                                                     \
    _Pragma("unroll") for (int g = 0; g < G::FN; ++g) aNN[g] = ok ? r0[oNN / 4 + 4 * g + KQ] : z4;                                        \
    _Pragma("unroll") for (int m = 0; m < G::TN; ++m) tNN[m] = ok ? rf[oNN + 16 * G::FN + 4 * m + KQ] : 0.f;                              \
  }

// KTUP_Q_DMA_OFFSETS(G, SOFF, W, LANE): declares SOFF[G::DPW], this lane's float4 of every DMA piece of its wave W: byte offset inside a
// tile (0xffffffff: the piece ends before this lane).
#define KTUP_Q_DMA_OFFSETS(G, SOFF, W, LANE)                                                                                              \
  uint32_t SOFF[G::DPW];                                                                                                                  \
  _Pragma("unroll") for (int k = 0; k < G::DPW; ++k) {                                                                                    \
    const int slot = 64 * (W + 4 * k) + LANE;                                                                                             \
    SOFF[k] = slot < G::TSLOTS ? (uint32_t)slot * 16u : 0xffffffffu;                                                                      \
  }

// KTUP_Q_TILE_DMA(G, TABLE, N_ITEMS, ROW0, DST, SOFF): the 16 consecutive rows of TABLE from ROW0 on -> the LDS tile whose piece of this
// wave starts at DST (tiles past the table's end re-read its last row: their items are masked out by the caller, the operands only
// have to be finite).
#define KTUP_Q_TILE_DMA(G, TABLE, N_ITEMS, ROW0, DST, SOFF)                                                                               \
  {                                                                                                                                       \
    const int64_t row0 = ROW0;                                                                                                            \
    const char* src = reinterpret_cast<const char*>(TABLE + row0 * G::GROW);                                                              \
    v4* dst = DST;                                                                                                                        \
    const bool tail = row0 + IBT > N_ITEMS;                             /* (uniform) */                                                   \
    _Pragma("unroll") for (int k = 0; k < G::DPW; ++k) {                                                                                  \
      if (SOFF[k] == 0xffffffffu) continue;                                                                                               \
      const char* from = src + SOFF[k];                                                                                                   \
      if (tail) {                                                                                                                         \
        const uint32_t slot = SOFF[k] >> 4, row = slot / G::ROW4, c = slot - row * G::ROW4;                                               \
        const int64_t r = row0 + row < N_ITEMS ? row0 + row : N_ITEMS - 1;                                                                \
        from = reinterpret_cast<const char*>(TABLE + r * G::GROW + 4 * c);                                                                \
      }                                                                                                                                   \
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)from,                                               \
                                       (__attribute__((address_space(3))) void*)(dst + 256 * k), 16, 0, 0);                               \
    }                                                                                                                                     \
  }

// KTUP_Q_TILE_MFMA(G, IROW, KQ): declares accAA, accS, accAN, accNN (and its working names, in the scope it stands in) and runs 16 users (the operands of KTUP_Q_USER_OPS) x the 16 items of a
// staged tile through the chain; IROW (a const v4*): this lane's item row of the tile (lane (KQ, item j)).
// B operands one step ahead of the MFMAs that use them (two register sets): left to itself the compiler re-uses ONE set and
// every group of MFMAs waits out an LDS round trip (measured: the MFMAs + reads alone took 120 us of a 68 us pipe time).
// Steps: AA's whole blocks, AA's remaining quads, the [L ; Nx] blocks (S, AN and -- the first FN -- NN), their remaining quads
// (S, AN), NN's remaining quads.
#define KTUP_Q_TILE_MFMA(G, IROW, KQ)                                                                                                     \
  const v4* ib = (IROW) + KQ;                                           /* k-quad KQ of every 16-block */                                 \
  v4 accAA = (v4){0.f, 0.f, 0.f, 0.f}, accS = accAA, accAN = accAA, accNN = accAA;                                                        \
  const float* ibf = reinterpret_cast<const float*>(IROW) + KQ;       /* element KQ of a k-quad */                                        \
  constexpr int S0 = G::FA, S1 = S0 + G::TA, S2 = S1 + G::FS, S3 = S2 + G::TS, NSTEP = S3 + G::TN;                                        \
  constexpr int SF = 4 * G::SOFF4;                                    /* float offset of [L ; Nx] inside a row */                         \
  auto bsrc = [&](int s) -> v4 {                                                                                                          \
    if (s < S0) return ib[4 * s];                                                                                                         \
    if (s < S1) return (v4){ibf[16 * G::FA + 4 * (s - S0)], 0.f, 0.f, 0.f};                                                               \
    if (s < S2) return ib[G::SOFF4 + 4 * (s - S1)];                                                                                       \
    if (s < S3) return (v4){ibf[SF + 16 * G::FS + 4 * (s - S2)], 0.f, 0.f, 0.f};                                                          \
    return (v4){ibf[SF + 16 * G::FN + 4 * (s - S3)], 0.f, 0.f, 0.f};                                                                      \
  };                                                                                                                                      \
  v4 bcur = bsrc(0);                                                                                                                      \
  _Pragma("unroll") for (int s = 0; s < NSTEP; ++s) {                                                                                     \
    v4 bnext = bcur;                                                                                                                      \
    if (s + 1 < NSTEP) bnext = bsrc(s + 1);                                                                                               \
    __builtin_amdgcn_sched_barrier(0);                                /* the read stays ahead of the MFMAs below */                       \
    if (s < S0) {                                                                                                                         \
      _Pragma("unroll") for (int c = 0; c < 4; ++c) accAA = __builtin_amdgcn_mfma_f32_16x16x4f32(aAA[s][c], bcur[c], accAA, 0, 0, 0);     \
    } else if (s < S1) {                                                                                                                  \
      accAA = __builtin_amdgcn_mfma_f32_16x16x4f32(tAA[s - S0], bcur[0], accAA, 0, 0, 0);                                                 \
    } else if (s < S2) {                                                                                                                  \
      const int g = s - S1;                                                                                                               \
      _Pragma("unroll") for (int c = 0; c < 4; ++c) {                                                                                     \
        accS = __builtin_amdgcn_mfma_f32_16x16x4f32(aS[g][c], bcur[c], accS, 0, 0, 0);                                                    \
        accAN = __builtin_amdgcn_mfma_f32_16x16x4f32(aAN[g][c], bcur[c], accAN, 0, 0, 0);                                                 \
        if (g < G::FN) accNN = __builtin_amdgcn_mfma_f32_16x16x4f32(aNN[g][c], bcur[c], accNN, 0, 0, 0);                                  \
      }                                                                                                                                   \
    } else if (s < S3) {                                                                                                                  \
      accS = __builtin_amdgcn_mfma_f32_16x16x4f32(tS[s - S2], bcur[0], accS, 0, 0, 0);                                                    \
      accAN = __builtin_amdgcn_mfma_f32_16x16x4f32(tAN[s - S2], bcur[0], accAN, 0, 0, 0);                                                 \
    } else {                                                                                                                              \
      accNN = __builtin_amdgcn_mfma_f32_16x16x4f32(tNN[s - S3], bcur[0], accNN, 0, 0, 0);                                                 \
    }                                                                                                                                     \
    __builtin_amdgcn_sched_barrier(0);                                                                                                    \
    bcur = bnext;                                                                                                                         \
  }

// |a|^2 - 2 s (a.n) + s^2 |n|^2 from the user's scalars us4, the item's is4 and the four cross terms of the pair
KTUP_DEV float q_score(const v4& us4, const v4& is4, float cS, float cAA, float cAN, float cNN) {
  const float sv = (us4[0] + cS) - is4[0];
  const float aa = (us4[1] + is4[1]) + cAA;
  const float an = (us4[2] + cAN) - is4[2];
  const float nn = (us4[3] + is4[3]) + cNN;
  return fmaf(sv * sv, nn, fmaf(-2.f * sv, an, aa));
}

}  // namespace
}  // namespace ktup
